// ann_pack_check.cpp -- CPU check of csrc/ik_ann_pack.cpp, built with
// -fsanitize=address,undefined by tests/test_ann_pack_cpu.py.
//
// Every destination is allocated with exactly its size function's bytes, so an
// overrun is a sanitizer report.  The orders are checked by the inverse mapping:
// every destination index is decoded to its (k, c) coordinates and must hold
// W[k][c] (0 in the padding), and every W element must be met once per plane.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "ik_ann_pack.h"
#include "ikhip.h"

using namespace ikhip;

static int g_fail = 0;
#define CHECK(cond, ...)                         \
  do {                                           \
    if (!(cond)) {                               \
      if (++g_fail <= 20) {                      \
        std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
        std::printf(__VA_ARGS__);                \
        std::printf("\n");                       \
      }                                          \
    }                                            \
  } while (0)

static size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

// dist 0: N(0, 0.1); 1: +-2^u, u uniform in [-20, 4]
static std::vector<float> weights(int k, int n, int dist, unsigned seed) {
  std::mt19937 rng(seed);
  std::normal_distribution<float> nd(0.0f, 0.1f);
  std::uniform_real_distribution<float> ud(-20.0f, 4.0f);
  std::vector<float> W((size_t)k * n);
  for (float &w : W) w = dist == 0 ? nd(rng) : ((rng() & 1) ? -1.0f : 1.0f) * std::exp2(ud(rng));
  return W;
}

static float bf16_value(uint16_t h) {
  const uint32_t u = (uint32_t)h << 16;
  float x;
  std::memcpy(&x, &u, 4);
  return x;
}

// Coordinates of element e of a 16x16x32 fragment stream with P planes.
struct Frag16 {
  int kk, c, p;
};
static Frag16 decode16(size_t e, int P, int G32) {
  const int j = e % 8, lane = (e / 8) % 64, p = (e / 512) % P, fh = (e / (512 * P)) % 2;
  const int g = (e / (1024 * P)) % G32, nt = (int)(e / ((size_t)1024 * P * G32));
  return {32 * g + 8 * (lane >> 4) + j, 32 * nt + 16 * fh + (lane & 15), p};
}

static void check_fp32(int k, int n) {
  const std::vector<float> W = weights(k, n, 0, 1000 + k + n);
  const size_t cnt = ann_packed_floats(k, n);
  std::unique_ptr<float[]> d(new float[cnt]);
  ann_pack_layer(W.data(), k, n, d.get());
  const int G = (k + 7) / 8;
  std::vector<int> met((size_t)k * n, 0);
  for (size_t e = 0; e < cnt; ++e) {
    const int s = e % 4, lane = (e / 4) % 64, g = (e / 256) % G, nt = (int)(e / ((size_t)256 * G));
    const int kk = 8 * g + 4 * (lane >> 5) + s, c = 32 * nt + (lane & 31);
    if (kk < k && c < n) {
      ++met[(size_t)kk * n + c];
      CHECK(d[e] == W[(size_t)kk * n + c], "fp32 (%d,%d) element %zu is not W[%d][%d]", k, n, e,
            kk, c);
    } else {
      CHECK(d[e] == 0.0f && !std::signbit(d[e]), "fp32 (%d,%d) padding %zu not 0", k, n, e);
    }
  }
  for (size_t i = 0; i < met.size(); ++i)
    CHECK(met[i] == 1, "fp32 (%d,%d) W[%zu] met %d times", k, n, i, met[i]);
}

// The planes of a bf16x6 operand, already gathered per weight: sum exact, and
// the planes in falling order (hi within 2^-8 of x, hi + mid within 2^-16).
static void check_bf16_planes(const char *what, int k, int n, const std::vector<float> &W,
                              const std::vector<float> (&pl)[3], const std::vector<int> &met) {
  for (size_t i = 0; i < W.size(); ++i) {
    CHECK(met[i] == 3, "%s (%d,%d) W[%zu] met %d times", what, k, n, i, met[i]);
    const float x = W[i], hi = pl[0][i], mid = pl[1][i], lo = pl[2][i];
    CHECK((double)hi + (double)mid + (double)lo == (double)x, "%s (%d,%d) W[%zu] sum", what, k, n, i);
    CHECK(std::fabs(x - hi) <= std::fabs(x) * 0x1p-8f, "%s (%d,%d) W[%zu] hi plane", what, k, n, i);
    CHECK(std::fabs((x - hi) - mid) <= std::fabs(x) * 0x1p-16f, "%s (%d,%d) W[%zu] mid plane", what,
          k, n, i);
  }
}

static void check_x(int k, int n, int dist) {
  const std::vector<float> W = weights(k, n, dist, 2000 + k + n);
  const size_t cnt = ann_x_bytes(k, n) / 2;
  std::unique_ptr<uint16_t[]> d(new uint16_t[cnt]);
  ann_pack_layer_x(W.data(), k, n, d.get());
  const int G32 = (k + 31) / 32;
  CHECK(cnt == (size_t)1024 * 3 * G32 * ((n + 31) / 32), "ann_x_bytes(%d,%d)", k, n);
  std::vector<float> pl[3] = {std::vector<float>(W.size()), std::vector<float>(W.size()),
                              std::vector<float>(W.size())};
  std::vector<int> met(W.size(), 0);
  for (size_t e = 0; e < cnt; ++e) {
    const Frag16 f = decode16(e, 3, G32);
    if (f.kk < k && f.c < n) {
      ++met[(size_t)f.kk * n + f.c];
      pl[f.p][(size_t)f.kk * n + f.c] = bf16_value(d[e]);
    } else {
      CHECK(d[e] == 0, "bf16x6 (%d,%d) padding %zu not 0", k, n, e);
    }
  }
  check_bf16_planes("bf16x6", k, n, W, pl, met);
}

static void check_big_x(int k, int n, int dist) {
  const std::vector<float> W = weights(k, n, dist, 3000 + k + n);
  const size_t cnt = ann_big_x_bytes(k, n) / 2;
  std::unique_ptr<uint16_t[]> d(new uint16_t[cnt]);
  ann_big_pack_x(W.data(), k, n, d.get());
  const int NP = (n + 127) / 128 * 128, KG = (k + 31) / 32;
  const size_t plane = (size_t)KG * NP * 32;
  CHECK(cnt == 3 * plane, "ann_big_x_bytes(%d,%d)", k, n);
  std::vector<float> pl[3] = {std::vector<float>(W.size()), std::vector<float>(W.size()),
                              std::vector<float>(W.size())};
  std::vector<int> met(W.size(), 0);
  for (size_t e = 0; e < cnt; ++e) {
    const int p = (int)(e / plane), kk = 32 * (int)((e % plane) / ((size_t)32 * NP)) + e % 32;
    const int c = (e / 32) % NP;
    if (kk < k && c < n) {
      ++met[(size_t)kk * n + c];
      pl[p][(size_t)kk * n + c] = bf16_value(d[e]);
    } else {
      CHECK(d[e] == 0, "layered bf16x6 (%d,%d) padding %zu not 0", k, n, e);
    }
  }
  check_bf16_planes("layered bf16x6", k, n, W, pl, met);
}

static void check_h(int k, int n, int dist) {
  const std::vector<float> W = weights(k, n, dist, 4000 + k + n);
  const int s = ann_h_scale_exp(W.data(), k, n);
  float mx = 0.0f;
  for (float w : W) mx = std::fmax(mx, std::fabs(std::ldexp(w, s)));
  CHECK(mx >= 0x1p13f && mx < 0x1p14f, "fp16x3 (%d,%d) scaled max %g", k, n, mx);
  const size_t cnt = ann_h_bytes(k, n) / 2;
  std::unique_ptr<_Float16[]> d(new _Float16[cnt]);
  ann_pack_layer_h(W.data(), k, n, s, d.get());
  const int G32 = (k + 31) / 32;
  CHECK(cnt == (size_t)1024 * 2 * G32 * ((n + 31) / 32), "ann_h_bytes(%d,%d)", k, n);
  std::vector<float> pl[2] = {std::vector<float>(W.size()), std::vector<float>(W.size())};
  std::vector<int> met(W.size(), 0);
  for (size_t e = 0; e < cnt; ++e) {
    const Frag16 f = decode16(e, 2, G32);
    if (f.kk < k && f.c < n) {
      ++met[(size_t)f.kk * n + f.c];
      pl[f.p][(size_t)f.kk * n + f.c] = (float)d[e];
    } else {
      CHECK((float)d[e] == 0.0f, "fp16x3 (%d,%d) padding %zu not 0", k, n, e);
    }
  }
  for (size_t i = 0; i < W.size(); ++i) {
    CHECK(met[i] == 2, "fp16x3 (%d,%d) W[%zu] met %d times", k, n, i, met[i]);
    const double x = std::ldexp((double)W[i], s), hi = pl[0][i], lo = pl[1][i];
    // hi within half an fp16 ulp of x (relative 2^-11, 2^-25 in the subnormal range);
    // the sum within half an ulp of the residual, which is at most 4: 2^-10
    CHECK(std::fabs(x - hi) <= std::fmax(std::fabs(x) * 0x1p-11, 0x1p-25),
          "fp16x3 (%d,%d) W[%zu] hi plane", k, n, i);
    CHECK(std::fabs(x - (hi + lo)) <= 0x1p-10, "fp16x3 (%d,%d) W[%zu]: |x - (hi + lo)| = %g", k, n,
          i, std::fabs(x - (hi + lo)));
  }
}

static void check_h_exponent_edges() {
  std::vector<float> W(33 * 40, 0.0f);
  CHECK(ann_h_scale_exp(W.data(), 33, 40) == 0, "all-zero layer: exponent not 0");
  W[17] = 0.25f;
  W[700] = -INFINITY;
  CHECK(ann_h_scale_exp(W.data(), 33, 40) == 0, "layer with inf: exponent not 0");
}

// The largest |w| of a halvable layer swept over 2^-100 .. 2^100 (times 1.9995,
// the mantissa that rounds up first), the other weights down to 2^-12 of it,
// through ann_pack_section.  While the pre-scale exponent is within
// +-kAnnHMaxScaleExp the planes are built, finite, and hi + lo is the scaled
// weight to 2^-21 of the largest; past it they are not built (the section stays
// zero and the layer runs fp32) -- a clamped exponent would leave the largest
// weights above fp16's 65504 from 2^75 on.
static void check_h_scale_sweep() {
  const int32_t dims[] = {3, 33, 40, 4}, acts[] = {IK_ACT_TANH, IK_ACT_TANH, IK_ACT_LINEAR};
  const AnnLayout L(3, dims, acts, true);
  CHECK(L.halvable[1], "sweep layout: layer 1 not halvable");
  const int k = 33, n = 40, G32 = 2;
  const std::vector<float> b(n, 0.0f);
  std::mt19937 rng(77);
  std::uniform_real_distribution<float> ud(-12.0f, 0.0f);
  for (int E = -100; E <= 100; ++E) {
    std::vector<float> W((size_t)k * n);
    for (float &w : W) w = std::ldexp(((rng() & 1) ? -1.0f : 1.0f) * std::exp2(ud(rng)), E);
    W[5 * n + 7] = std::ldexp(-1.9995f, E);
    W[32 * n + 39] = std::ldexp(1.9995f, E);
    std::unique_ptr<char[]> sec(new char[L.section_bytes(1)]());
    bool built = true;
    const int s = ann_pack_section(L, 1, W.data(), b.data(), sec.get(), &built);
    const bool inside = 13 - E >= -kAnnHMaxScaleExp && 13 - E <= kAnnHMaxScaleExp;
    CHECK(built == inside, "sweep 2^%d: planes %s", E, built ? "built" : "not built");
    CHECK(s == (inside ? 13 - E : 0), "sweep 2^%d: exponent %d", E, s);
    const _Float16 *d = reinterpret_cast<const _Float16 *>(sec.get() + (L.hoff[1] - L.woff[1]));
    const size_t cnt = ann_h_bytes(k, n) / 2;
    std::vector<double> hi(W.size(), 0.0), lo(W.size(), 0.0);
    for (size_t e = 0; e < cnt; ++e) {
      const float v = (float)d[e];
      CHECK(std::isfinite(v), "sweep 2^%d: element %zu is %g", E, e, v);
      CHECK(built || v == 0.0f, "sweep 2^%d: planes not built but element %zu is %g", E, e, v);
      const Frag16 f = decode16(e, 2, G32);
      if (f.kk < k && f.c < n) (f.p ? lo : hi)[(size_t)f.kk * n + f.c] = v;
    }
    if (!built) continue;
    const double mx = std::ldexp(1.9995, E + s);
    for (size_t i = 0; i < W.size(); ++i) {
      const double x = std::ldexp((double)W[i], s);
      CHECK(std::fabs(x - (hi[i] + lo[i])) <= mx * 0x1p-21, "sweep 2^%d W[%zu]: |x - (hi + lo)| = %g",
            E, i, std::fabs(x - (hi[i] + lo[i])));
    }
  }
}

// The operands of a layout, in address order: ascending, aligned, disjoint.
static void check_sections(const char *what, const AnnLayout &L) {
  size_t end = 0;
  auto next = [&](size_t off, size_t bytes, const char *op, int l) {
    CHECK(off % 256 == 0, "%s layer %d %s not 256-aligned", what, l, op);
    CHECK(off >= end, "%s layer %d %s overlaps its predecessor", what, l, op);
    end = off + bytes;
  };
  for (int l = 0; l < L.n_layers(); ++l) {
    const int k = L.dims[l], n = L.dims[l + 1];
    const size_t w0 = L.woff[l];
    next(L.woff[l], ann_packed_floats(k, n) * 4, "weights", l);
    next(L.boff[l], (size_t)L.np(l) * 4, "bias", l);
    if (L.splittable[l])
      next(L.xoff[l], L.big ? ann_big_x_bytes(k, n) : ann_x_bytes(k, n), "bf16x6 planes", l);
    if (L.halvable[l]) next(L.hoff[l], ann_h_bytes(k, n), "fp16x3 planes", l);
    CHECK(L.section_bytes(l) == up256(end) - w0, "%s layer %d section_bytes", what, l);
  }
  CHECK(L.total == up256(end), "%s total %zu, last operand ends at %zu", what, L.total, end);
}

static void check_flags(const char *what, const AnnLayout &L, int s0, int s1, int h0, int h1) {
  for (int l = 0; l < L.n_layers(); ++l) {
    CHECK(!!L.splittable[l] == (l >= s0 && l <= s1), "%s splittable[%d]", what, l);
    CHECK(!!L.halvable[l] == (l >= h0 && l <= h1), "%s halvable[%d]", what, l);
  }
}

static void check_layout() {
  {  // the reference model 3 -> 12 x 500 -> 4
    std::vector<int32_t> dims = {3}, a_tanh(13, IK_ACT_TANH), a_relu(13, IK_ACT_RELU);
    for (int i = 0; i < 12; ++i) dims.push_back(500);
    dims.push_back(4);
    a_tanh[12] = a_relu[12] = IK_ACT_LINEAR;
    const AnnLayout T(13, dims.data(), a_tanh.data(), true);
    CHECK(!T.big && !T.wide && T.act_min == 0, "reference model: big / wide / act_min");
    check_sections("reference model", T);
    check_flags("reference model", T, 1, 11, 1, 11);
    const AnnLayout R(13, dims.data(), a_relu.data(), true);
    check_sections("relu model", R);
    check_flags("relu model", R, 1, 11, 1, 0);
    const AnnLayout N(13, dims.data(), a_tanh.data(), false);
    check_sections("model without planes", N);
    check_flags("model without planes", N, 1, 0, 1, 0);
    CHECK(N.total < R.total && R.total < T.total, "plane bytes missing from total");

    // one section through ann_pack_section against the packers
    const std::vector<float> W = weights(500, 500, 0, 7), b = weights(1, 500, 0, 8);
    std::unique_ptr<char[]> sec(new char[T.section_bytes(3)]());
    const int e = ann_pack_section(T, 3, W.data(), b.data(), sec.get());
    CHECK(e == ann_h_scale_exp(W.data(), 500, 500), "ann_pack_section exponent");
    std::unique_ptr<char[]> ref(new char[ann_x_bytes(500, 500)]);
    ann_pack_layer(W.data(), 500, 500, reinterpret_cast<float *>(ref.get()));
    CHECK(!std::memcmp(sec.get(), ref.get(), ann_packed_floats(500, 500) * 4), "section weights");
    CHECK(!std::memcmp(sec.get() + (T.boff[3] - T.woff[3]), b.data(), 500 * 4), "section bias");
    for (int c = 500; c < 512; ++c)
      CHECK(reinterpret_cast<float *>(sec.get() + (T.boff[3] - T.woff[3]))[c] == 0.0f, "bias pad");
    ann_pack_layer_x(W.data(), 500, 500, ref.get());
    CHECK(!std::memcmp(sec.get() + (T.xoff[3] - T.woff[3]), ref.get(), ann_x_bytes(500, 500)),
          "section bf16x6 planes");
    ann_pack_layer_h(W.data(), 500, 500, e, ref.get());
    CHECK(!std::memcmp(sec.get() + (T.hoff[3] - T.woff[3]), ref.get(), ann_h_bytes(500, 500)),
          "section fp16x3 planes");
  }
  {
    const int32_t dims[] = {3, 600, 4}, acts[] = {IK_ACT_TANH, IK_ACT_LINEAR};
    const AnnLayout L(2, dims, acts, true);
    CHECK(!L.big && L.wide && L.act_min == 0, "(3,600,4): big / wide / act_min");
    check_sections("(3,600,4)", L);
    check_flags("(3,600,4)", L, 1, 0, 1, 0);
  }
  {
    const int32_t dims[] = {3, 1100, 300, 4}, acts[] = {IK_ACT_TANH, IK_ACT_TANH, IK_ACT_LINEAR};
    const AnnLayout L(3, dims, acts, true);
    CHECK(L.big && L.wide, "(3,1100,300,4): big / wide");
    CHECK(L.act_min == (size_t)2 * 128 * 1120 * 4, "(3,1100,300,4): act_min %zu", L.act_min);
    check_sections("(3,1100,300,4)", L);
    check_flags("(3,1100,300,4)", L, 1, 1, 1, 0);
    CHECK(L.woff[2] - L.xoff[1] == up256(ann_big_x_bytes(1100, 300)), "(3,1100,300,4): planes' bytes");
    const std::vector<float> W = weights(1100, 300, 0, 9), b = weights(1, 300, 0, 10);
    std::unique_ptr<char[]> sec(new char[L.section_bytes(1)]());
    CHECK(ann_pack_section(L, 1, W.data(), b.data(), sec.get()) == 0, "layered section exponent");
    std::unique_ptr<char[]> ref(new char[ann_big_x_bytes(1100, 300)]);
    ann_big_pack_x(W.data(), 1100, 300, ref.get());
    CHECK(!std::memcmp(sec.get() + (L.xoff[1] - L.woff[1]), ref.get(), ann_big_x_bytes(1100, 300)),
          "layered section planes");
  }
  {
    std::vector<int32_t> dims = {3}, acts(25, IK_ACT_TANH);
    for (int i = 0; i < 24; ++i) dims.push_back(64);
    dims.push_back(4);
    const AnnLayout L(25, dims.data(), acts.data(), true);
    CHECK(L.big && L.act_min == (size_t)2 * 128 * 64 * 4, "25 layers of 64: big / act_min");
    check_sections("25 layers of 64", L);
    check_flags("25 layers of 64", L, 1, 23, 1, 0);
  }
}

int main() {
  const int fp32_shapes[][2] = {{1, 1},   {3, 12},    {7, 31},    {8, 32},
                                {9, 33},  {37, 250},  {500, 500}, {513, 1024}};
  for (const auto &s : fp32_shapes) check_fp32(s[0], s[1]);
  const int frag16_shapes[][2] = {{32, 64}, {33, 33}, {100, 37}, {500, 500}};
  const int big_shapes[][2] = {{37, 129}, {1100, 200}};
  for (int dist = 0; dist < 2; ++dist) {
    for (const auto &s : frag16_shapes) {
      check_x(s[0], s[1], dist);
      check_h(s[0], s[1], dist);
    }
    for (const auto &s : big_shapes) check_big_x(s[0], s[1], dist);
  }
  check_h_exponent_edges();
  check_h_scale_sweep();
  check_layout();
  if (g_fail) {
    std::printf("%d checks failed\n", g_fail);
    return 1;
  }
  std::printf("ann_pack_check ok\n");
  return 0;
}
