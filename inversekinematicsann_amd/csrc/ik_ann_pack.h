// ik_ann_pack.h -- host side of the ANN weight operands: the MFMA fragment
// orders the kernels read (ik_ann_kernel.h, ik_ann_big.hip) and the layout of a
// loaded model's device buffer.  Plain C++, no HIP header: the code is tested on
// the CPU (tests/test_ann_pack_cpu.py).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace ikhip {

// The fused kernel's caps; past them the layered path (ik_ann_big.hip) up to its own.
constexpr int kAnnMaxLayers = 24;
constexpr int kAnnMaxWidth = 1024;  // > 512: the wide build (ik_ann_w.hip), fp32 only
constexpr int kAnnBigMaxLayers = 4096;
constexpr int kAnnBigMaxWidth = 16384;

// W: one Dense layer's weights, float32 [k][n] row-major (the Keras kernel layout).
size_t ann_packed_floats(int k, int n);  // floats of one packed layer
void ann_pack_layer(const float *W, int k, int n, float *dst);
size_t ann_x_bytes(int k, int n);  // bytes of one layer's bf16x6 weight operand
void ann_pack_layer_x(const float *W, int k, int n, void *dst);
size_t ann_h_bytes(int k, int n);  // bytes of one layer's fp16x3 weight operand
int ann_h_scale_exp(const float *W, int k, int n);  // the weight pre-scale exponent
// The pre-scale exponents an fp16x3 operand is built for: 2^-e and the scaled
// bias stay well inside fp32.  Largest |w| from ~2^-47 to ~2^74; a layer outside
// runs fp32 in fp16x3 mode.
constexpr int kAnnHMaxScaleExp = 60;
void ann_pack_layer_h(const float *W, int k, int n, int scale_exp, void *dst);
// the layered path's bf16x6 weight planes: [plane][ceil(k / 32)][n rounded up to
// 128][32] bf16, ann_big_x_bytes(k, n) bytes
size_t ann_big_x_bytes(int k, int n);
void ann_big_pack_x(const float *W, int k, int n, void *dst);

// Where a model's operands lie in its one device buffer.  Layer l's section starts
// at woff[l] (256-byte aligned, like every operand): packed fp32 weights, the bias
// padded to whole column tiles, the bf16x6 planes (splittable), the fp16x3 planes (halvable).
//   big: past the fused kernel's caps, the layered path; wide: some width > 512.
//   splittable: a hidden layer after the first with more than one column tile,
//     on the fused kernel for widths <= 512 (ann_x_bytes) or on the layered
//     path (ann_big_x_bytes); none without `planes` (the split operands did not
//     fit the device: the split modes then run fp32).
//   halvable: splittable on the fused kernel, and the layer's input is bounded
//     (the layer before is tanh or sigmoid: fp16's range ends at 65504).
struct AnnLayout {
  AnnLayout(int n_layers, const int32_t *dims, const int32_t *acts, bool planes);
  bool big, wide;
  std::vector<int32_t> dims;                  // n_layers + 1 widths
  std::vector<size_t> woff, boff, xoff, hoff; // byte offsets (xoff / hoff: 0 without the operand)
  std::vector<char> splittable, halvable;
  size_t total;    // bytes of the buffer
  size_t act_min;  // layered path: its two activation buffers at one 128-row tile, else 0
  int n_layers() const { return (int)woff.size(); }
  int kp(int l) const { return (dims[l] + 7) / 8 * 8; }        // padded in-dim
  int np(int l) const { return (dims[l + 1] + 31) / 32 * 32; }  // padded out-dim
  size_t section_bytes(int l) const {
    return (l + 1 < n_layers() ? woff[l + 1] : total) - woff[l];
  }
};
// Layer l's section into dst (section_bytes(l), zeroed by the caller); returns
// the fp16x3 weight pre-scale exponent (0 for a layer that is not halvable).
// h_built: whether the fp16x3 planes were written -- not for a halvable layer
// whose exponent is outside +-kAnnHMaxScaleExp (its planes stay zero, unused).
int ann_pack_section(const AnnLayout &L, int l, const float *W, const float *b, char *dst,
                     bool *h_built = nullptr);

}  // namespace ikhip
