// ik_ann_pack.cpp -- the ANN weight operands' fragment orders and the model
// buffer's layout (ik_ann_pack.h).  Host only.
#include "ik_ann_pack.h"

#include <cmath>
#include <cstring>

#include "../../include/ikhip.h"

namespace ikhip {

size_t ann_packed_floats(int k, int n) {
  int kp = (k + 7) / 8 * 8, np = (n + 31) / 32 * 32;
  return (size_t)kp * np;
}

// dst[((nt*G + g)*64 + lane)*4 + s] = W[8g + 4*(lane>>5) + s][nt*32 + (lane&31)]
// -- the B fragment of v_mfma_f32_32x32x2_f32 for K-step s of group g, with the
// K order inside a group permuted to match the A fragment read (ds_read_b128 of
// 4 consecutive activations per lane half).
void ann_pack_layer(const float *W, int k, int n, float *dst) {
  int kp = (k + 7) / 8 * 8, np = (n + 31) / 32 * 32;
  int G = kp / 8, NT = np / 32;
  for (int nt = 0; nt < NT; ++nt)
    for (int g = 0; g < G; ++g)
      for (int lane = 0; lane < 64; ++lane)
        for (int s = 0; s < 4; ++s) {
          int kk = 8 * g + 4 * (lane >> 5) + s;
          int c = nt * 32 + (lane & 31);
          dst[(((size_t)nt * G + g) * 64 + lane) * 4 + s] =
              (kk < k && c < n) ? W[(size_t)kk * n + c] : 0.0f;
        }
}

// Round to nearest even, as v_cvt_pk_bf16_f32 does on the device.
static uint16_t bf16_rne(float x) {
  uint32_t u;
  std::memcpy(&u, &x, 4);
  if ((u & 0x7f800000u) == 0x7f800000u) return (uint16_t)(u >> 16);  // inf / nan (none expected)
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}

static float bf16_to_f32(uint16_t h) {
  uint32_t u = (uint32_t)h << 16;
  float x;
  std::memcpy(&x, &u, 4);
  return x;
}

// x = hi + mid + lo in bf16 (each residual exact in fp32), exactly as split3()
// splits the activations on the GPU; the planes `plane` elements apart.
static void bf16_split3(float x, uint16_t *d, size_t plane) {
  const uint16_t h = bf16_rne(x);
  const float r1 = x - bf16_to_f32(h);
  const uint16_t m = bf16_rne(r1);
  const float r2 = r1 - bf16_to_f32(m);
  d[0] = h;
  d[plane] = m;
  d[2 * plane] = bf16_rne(r2);
}

// The B-fragment order of v_mfma_f32_16x16x32_{bf16,f16}: for K step g (32 deep)
// of feature half fh of column tile nt, element j (0..7) of lane l is
// W[32g + 8*(l>>4) + j][32nt + 16fh + (l&15)], in P planes of 64 x 8 elements:
// plane p at dst[((((nt*G32 + g)*2 + fh)*P + p)*64 + l)*8 + j].  put(w, d) writes
// the planes of weight w (0 in the padding) to d[0], d[512], ...
template <int P, typename T, typename Put>
static void pack_frag16(const float *W, int k, int n, T *dst, Put put) {
  const int np = (n + 31) / 32 * 32, NT = np / 32, G32 = (k + 31) / 32;
  for (int nt = 0; nt < NT; ++nt)
    for (int g = 0; g < G32; ++g)
      for (int fh = 0; fh < 2; ++fh)
        for (int lane = 0; lane < 64; ++lane)
          for (int j = 0; j < 8; ++j) {
            const int kk = 32 * g + 8 * (lane >> 4) + j;
            const int c = nt * 32 + 16 * fh + (lane & 15);
            const float w = (kk < k && c < n) ? W[(size_t)kk * n + c] : 0.0f;
            put(w, dst + ((((size_t)nt * G32 + g) * 2 + fh) * P) * 64 * 8 + (size_t)lane * 8 + j);
          }
}

static size_t frag16_elems(int k, int n) {  // K padded to 32, N to 32
  return (size_t)((k + 31) / 32 * 32) * ((n + 31) / 32 * 32);
}

size_t ann_x_bytes(int k, int n) { return frag16_elems(k, n) * 6; }

// The bf16x6 weight operand: three bf16 planes (hi, mid, lo) in pack_frag16's
// order.  (An fp32 layout split in the kernel reads 4 B per weight instead of 6
// but measured slower at 64-point tiles: 30.5 vs 27.3 ms per 1M points, the VALU
// being the dearer.)
void ann_pack_layer_x(const float *W, int k, int n, void *dst) {
  pack_frag16<3>(W, k, n, static_cast<uint16_t *>(dst),
                 [](float w, uint16_t *d) { bf16_split3(w, d, 64 * 8); });
}

size_t ann_h_bytes(int k, int n) { return frag16_elems(k, n) * 4; }

// The power of two that brings the layer's largest |weight| to [2^13, 2^14):
// the fp16 planes then keep their full 11 bits down to weights ~2^-10 of the
// largest, and nothing comes near fp16's 65504.  Not clamped: an exponent past
// +-kAnnHMaxScaleExp means no fp16x3 operand (ann_pack_section), since a clamped
// one would leave the largest weights above 65504 (inf planes) or, at the other
// end, in fp16's subnormals.
int ann_h_scale_exp(const float *W, int k, int n) {
  float mx = 0.0f;
  for (size_t i = 0; i < (size_t)k * n; ++i) mx = std::fmax(mx, std::fabs(W[i]));
  if (!(mx > 0.0f) || !std::isfinite(mx)) return 0;
  int e = 0;
  std::frexp(mx, &e);  // mx in [2^(e-1), 2^e)
  return 14 - e;
}

// The fp16x3 weight operand: planes (hi, lo) of W * 2^scale_exp in pack_frag16's
// order, each rounded to nearest (the scaled weight and its residual are exact
// in fp32).
void ann_pack_layer_h(const float *W, int k, int n, int scale_exp, void *dst) {
  pack_frag16<2>(W, k, n, static_cast<_Float16 *>(dst), [scale_exp](float w, _Float16 *d) {
    const float x = std::ldexp(w, scale_exp);
    const _Float16 h = (_Float16)x;
    d[0] = h;
    d[64 * 8] = (_Float16)(x - (float)h);
  });
}

size_t ann_big_x_bytes(int k, int n) {
  return (size_t)3 * ((k + 31) / 32) * ((n + 127) / 128 * 128) * 32 * 2;
}

void ann_big_pack_x(const float *W, int k, int n, void *dst) {
  const int KG = (k + 31) / 32, NP = (n + 127) / 128 * 128;  // (whole 128-feature blocks)
  uint16_t *d = static_cast<uint16_t *>(dst);
  const size_t plane = (size_t)KG * NP * 32;
  for (int g = 0; g < KG; ++g)
    for (int c = 0; c < NP; ++c)
      for (int kk = 0; kk < 32; ++kk) {
        const int kr = 32 * g + kk;
        const float x = (kr < k && c < n) ? W[(size_t)kr * n + c] : 0.0f;
        bf16_split3(x, d + ((size_t)g * NP + c) * 32 + kk, plane);
      }
}

AnnLayout::AnnLayout(int n, const int32_t *d, const int32_t *acts, bool planes)
    : dims(d, d + n + 1), woff(n), boff(n), xoff(n, 0), hoff(n, 0), splittable(n, 0),
      halvable(n, 0), total(0), act_min(0) {
  big = n > kAnnMaxLayers;
  wide = false;
  for (int l = 0; l <= n; ++l) {
    big = big || dims[l] > kAnnMaxWidth;
    wide = wide || dims[l] > 512;
  }
  wide = wide || big;
  auto take = [this](size_t bytes) {  // the next operand's offset
    const size_t at = total;
    total = (total + bytes + 255) & ~(size_t)255;
    return at;
  };
  size_t ld = 8;  // floats per activation row of the layered path (ann_big_ld)
  for (int l = 0; l < n; ++l) {
    const int k = dims[l], w = dims[l + 1];
    splittable[l] = planes && (!wide || big) && l > 0 && np(l) / 32 > 1;
    halvable[l] = !big && splittable[l] &&
                  (acts[l - 1] == IK_ACT_TANH || acts[l - 1] == IK_ACT_SIGMOID);
    woff[l] = take(ann_packed_floats(k, w) * 4);
    boff[l] = take((size_t)np(l) * 4);
    if (splittable[l]) xoff[l] = take(big ? ann_big_x_bytes(k, w) : ann_x_bytes(k, w));
    if (halvable[l]) hoff[l] = take(ann_h_bytes(k, w));
    ld = (size_t)np(l) > ld ? (size_t)np(l) : ld;
  }
  if (big) act_min = 2 * 128 * ld * sizeof(float);
}

int ann_pack_section(const AnnLayout &L, int l, const float *W, const float *b, char *dst,
                     bool *h_built) {
  if (h_built) *h_built = false;
  const int k = L.dims[l], n = L.dims[l + 1];
  const size_t at = L.woff[l];
  ann_pack_layer(W, k, n, reinterpret_cast<float *>(dst));
  std::memcpy(dst + (L.boff[l] - at), b, (size_t)n * 4);
  if (L.splittable[l]) {
    if (L.big) ann_big_pack_x(W, k, n, dst + (L.xoff[l] - at));
    else ann_pack_layer_x(W, k, n, dst + (L.xoff[l] - at));
  }
  if (!L.halvable[l]) return 0;
  const int e = ann_h_scale_exp(W, k, n);
  if (e < -kAnnHMaxScaleExp || e > kAnnHMaxScaleExp) return 0;  // the layer stays fp32
  ann_pack_layer_h(W, k, n, e, dst + (L.hoff[l] - at));
  if (h_built) *h_built = true;
  return e;
}

}  // namespace ikhip
