// ik_ann.h -- the ANN solvers' device models and launchers: the fused kernels
// (ik_ann.hip, ik_ann_x.hip, ik_ann_w.hip through ik_ann_kernel.h) and the layered
// path for models outside their caps (ik_ann_big.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "ik_ann_pack.h"
#include "ik_launch.h"
#include "ik_types.h"

namespace ikhip {

// A scaled ANN input that overflowed fp32 (a point ~1e39 scales away) in front of
// a bounded first layer (tanh / sigmoid): +-FLT_MAX saturates every real column
// exactly as +-inf would, but times the zero weights of the padded columns it is
// 0, not inf * 0 = NaN, which the next layer's padded K would spread over the row.
// NaN stays NaN.  In front of relu / linear the infinity itself goes in.
__device__ __forceinline__ float ann_input(double x, bool bounded) {
  const float v = (float)x;
  return (bounded && fabsf(v) == __builtin_inff()) ? copysignf(3.402823466e38f, v) : v;
}

// (the caps kAnnMaxLayers / kAnnMaxWidth and the weight packing: ik_ann_pack.h)
struct AnnModelDev {
  int n_layers;
  int kp[kAnnMaxLayers];  // padded in-dim (multiple of 8)
  int np[kAnnMaxLayers];  // padded out-dim (multiple of 32)
  int act[kAnnMaxLayers];
  const float4 *wp[kAnnMaxLayers];  // packed weights (ann_pack_layer)
  const void *wx[kAnnMaxLayers];    // split modes: the layer's weight operand, else null
  float xinv[kAnnMaxLayers];        // fp16x3: 2^-k, k the layer's weight pre-scale exponent
  int xmode;                        // 0 fp32, 1 bf16x6, 2 fp16x3 (IK_ANN_*)
  const float *bias[kAnnMaxLayers];
  double xm[3], xs[3], ym[4], ys[4];
};
size_t ann_debug_words();  // u64 slots of the diagnostic stamp buffer
void launch_ann(const AnnModelDev &m, const RobotDev &r, const double *pts, int64_t n,
                float *ang, double *fk_err, bool check_limits, DevStats *S, hipStream_t st,
                unsigned long long *dbg);
void launch_ann_wide(const AnnModelDev &m, const RobotDev &r, const double *pts, int64_t n,
                     float *ang, double *fk_err, bool check_limits, DevStats *S, hipStream_t st,
                     unsigned long long *dbg);

// Models outside the fused kernel's caps (more than kAnnMaxLayers layers or a
// layer wider than kAnnMaxWidth): layer at a time through HBM (ik_ann_big.hip),
// fp32, or bf16x6 for the hidden layers after the first in a split mode, up to
// kAnnBigMaxLayers layers of kAnnBigMaxWidth.
struct AnnBigLayer {
  int kp, np, act;   // padded in-dim (multiple of 8), padded out-dim (multiple of 32)
  const float *wp;   // packed weights (ann_pack_layer order)
  const float *bias; // np floats, zero past the layer's width
  const uint16_t *wx = nullptr;  // bf16x6 planes (ann_big_pack_x), hidden layers only
};
struct AnnBigModel {
  std::vector<AnnBigLayer> layers;
  double xm[3], xs[3], ym[4], ys[4];
};
// floats per activation row (the widest padded layer, at least 8)
size_t ann_big_ld(const AnnBigModel &m);
// rows per chunk that fit two activation buffers in act_bytes (multiple of 128)
int64_t ann_big_rows(const AnnBigModel &m, size_t act_bytes);
// act: 2 * chunk_rows * ann_big_ld(m) floats
void launch_ann_big(const AnnBigModel &m, const RobotDev &r, const double *pts, int64_t n,
                    float *ang, double *fk_err, bool check_limits, DevStats *S, hipStream_t st,
                    float *act, int64_t chunk_rows, int xmode = 0);

}  // namespace ikhip
