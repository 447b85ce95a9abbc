// chain_jac_check.cpp -- CPU check of csrc/ik_chain_jac.h (the forward-kinematics
// chain with its Jacobian that the refine kernel and the training loss's FK term
// compile) and of csrc/ik_row.h's wrap_pi.  Stand-alone, built with AddressSanitizer +
// UndefinedBehaviorSanitizer by tests/test_chain_jac_cpu.py and run directly.
//
//   chain_jac_check            the wrap's check, then "chain_jac_check ok"
//   chain_jac_check IN OUT     also runs fk_chain_jac on the rows of the file IN, raw
//       float64: the number of tables, then per table the number of rows n, the DH table
//       (16: theta, d, a, alpha), jc (16, fk_trip_consts' layout) and n rows of
//       theta[4] sin[4] cos[4].  Writes per row x y z j0x j0y j1x j1y j1z .. j3z (14, raw
//       float64) to OUT; the test compares them byte for byte with the numpy restatement.
//
// The rows are also checked by what they have to be, not by a copy of the chain: the
// effector is the translation of the product of the four 4 x 4 DH matrices
// Rz(theta) Tz(d) Tx(a) Rx(alpha), formed here in long double, and column i of the
// Jacobian is the geometric one of a revolute joint, z_{i-1} x (p - o_{i-1}), with
// z_{i-1} and o_{i-1} the z axis and the origin of the frame before joint i in that
// same long double product.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "ik_chain_jac.h"

using namespace ikhip;

static int g_fail = 0;
#define CHECK(cond, ...)                                 \
  do {                                                   \
    if (!(cond)) {                                       \
      if (++g_fail <= 20) {                              \
        std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
        std::printf(__VA_ARGS__);                        \
        std::printf("\n");                               \
      }                                                  \
    }                                                    \
  } while (0)

typedef long double ld;
static const double kPiD = 3.141592653589793;

struct M4 {
  ld m[4][4];
};
static M4 ident() {
  M4 r = {};
  for (int i = 0; i < 4; ++i) r.m[i][i] = 1.0L;
  return r;
}
static M4 mul(const M4 &a, const M4 &b) {
  M4 r = {};
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j)
      for (int k = 0; k < 4; ++k) r.m[i][j] += a.m[i][k] * b.m[k][j];
  return r;
}
// T[i]: the frame after joint i (T[0] the base); rows of dh: theta (not read), d, a, alpha
static void frames_ld(const double *dh, const double th[4], M4 T[5]) {
  T[0] = ident();
  for (int i = 0; i < 4; ++i) {
    M4 rz = ident(), tz = ident(), tx = ident(), rx = ident();
    const ld t = (ld)th[i], al = (ld)dh[12 + i];
    rz.m[0][0] = cosl(t), rz.m[0][1] = -sinl(t);
    rz.m[1][0] = sinl(t), rz.m[1][1] = cosl(t);
    tz.m[2][3] = (ld)dh[4 + i];
    tx.m[0][3] = (ld)dh[8 + i];
    rx.m[1][1] = cosl(al), rx.m[1][2] = -sinl(al);
    rx.m[2][1] = sinl(al), rx.m[2][2] = cosl(al);
    T[i + 1] = mul(T[i], mul(mul(mul(rz, tz), tx), rx));
  }
}

// One table's rows.  The bound is train_fk_row_check.cpp's rule: 50 x one float64
// rounding (1.1e-16 relative) of a value of the checked quantity's size.  The
// effector's entries are at most the chain's total length L = sum |a_i| + |d_i|, and
// so are the Jacobian's: |z x (p - o)| <= |p - o| <= L.  The sines and cosines the
// test passes in are libm's, within one such rounding of the long double ones.
static void run_table(const double *dh, const double *jc, const double *rows, int64_t n,
                      double *out, double *worst_p, double *worst_j) {
  double L = 0.0;
  for (int i = 0; i < 4; ++i) L += std::fabs(dh[4 + i]) + std::fabs(dh[8 + i]);
  const double bound = 50 * (DBL_EPSILON / 2) * L;
  for (int64_t r = 0; r < n; ++r) {
    const double *th = rows + 12 * r, *s = th + 4, *c = th + 8;
    const ChainJac f = fk_chain_jac(jc, s, c);
    const RefineJ &J = f.J;
    const double got[14] = {f.x,   f.y,   f.z,   J.j0x, J.j0y, J.j1x, J.j1y,
                            J.j1z, J.j2x, J.j2y, J.j2z, J.j3x, J.j3y, J.j3z};
    for (int k = 0; k < 14; ++k) out[14 * r + k] = got[k];
    M4 T[5];
    frames_ld(dh, th, T);
    const ld p[3] = {T[4].m[0][3], T[4].m[1][3], T[4].m[2][3]};
    for (int k = 0; k < 3; ++k) {
      const double d = std::fabs((double)((ld)got[k] - p[k]));
      *worst_p = d > *worst_p ? d : *worst_p;
      CHECK(d <= bound, "row %lld: effector[%d] %.17g, long double %.17Lg (bound %.3g)",
            (long long)r, k, got[k], p[k], bound);
    }
    const double *col[4] = {&got[3], &got[5], &got[8], &got[11]};
    for (int i = 0; i < 4; ++i) {
      const ld z[3] = {T[i].m[0][2], T[i].m[1][2], T[i].m[2][2]};
      const ld v[3] = {p[0] - T[i].m[0][3], p[1] - T[i].m[1][3], p[2] - T[i].m[2][3]};
      const ld want[3] = {z[1] * v[2] - z[2] * v[1], z[2] * v[0] - z[0] * v[2],
                          z[0] * v[1] - z[1] * v[0]};
      if (i == 0) CHECK(want[2] == 0.0L, "column 1 has a z part: %.17Lg", want[2]);
      for (int k = 0; k < (i == 0 ? 2 : 3); ++k) {
        const double d = std::fabs((double)((ld)col[i][k] - want[k]));
        *worst_j = d > *worst_j ? d : *worst_j;
        CHECK(d <= bound, "row %lld: J[%d][%d] %.17g, geometric %.17Lg (bound %.3g)",
              (long long)r, k, i, col[i][k], want[k], bound);
      }
    }
  }
}

static std::vector<double> read_all(const char *path) {
  std::vector<double> v;
  std::FILE *f = std::fopen(path, "rb");
  if (!f) return v;
  double buf[1024];
  size_t got;
  while ((got = std::fread(buf, sizeof(double), 1024, f)) > 0) v.insert(v.end(), buf, buf + got);
  std::fclose(f);
  return v;
}

static int run_file(const char *in, const char *outp) {
  const std::vector<double> v = read_all(in);
  std::vector<double> out;
  size_t at = 1;
  if (v.empty()) {
    std::printf("cannot read %s\n", in);
    return 1;
  }
  long long total = 0;
  double worst_p = 0.0, worst_j = 0.0;
  for (int t = 0; t < (int)v[0]; ++t) {
    if (at + 33 > v.size()) break;
    const int64_t n = (int64_t)v[at];
    if (n < 0 || at + 33 + 12 * (size_t)n > v.size()) break;
    const size_t base = out.size();
    out.resize(base + 14 * (size_t)n);
    run_table(&v[at + 1], &v[at + 17], v.data() + at + 33, n, out.data() + base, &worst_p,
              &worst_j);
    at += 33 + 12 * (size_t)n;
    total += n;
  }
  if (at != v.size()) {
    std::printf("%s: %zu doubles, the tables end at %zu\n", in, v.size(), at);
    return 1;
  }
  std::FILE *f = std::fopen(outp, "wb");
  if (!f || std::fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) {
    std::printf("cannot write %s\n", outp);
    return 1;
  }
  std::fclose(f);
  std::printf("rows %lld: worst |effector - long double| %.3e, worst |J - geometric| %.3e\n", total,
              worst_p, worst_j);
  return 0;
}

// The wrap on angles beyond +-2 pi (where only it keeps sincos_fk valid): the result
// lies within [-pi, pi] and is congruent to the input, as train_fk_row_check.cpp holds
// the wrap of its rows.
static void check_wrap() {
  uint64_t x = 88172645463325252ull;
  auto uni = [&](double lo, double hi) {
    x ^= x << 13, x ^= x >> 7, x ^= x << 17;  // xorshift64
    return lo + (double)(x >> 11) * 0x1p-53 * (hi - lo);
  };
  int beyond = 0;
  for (int i = 0; i < 4000; ++i) {
    const double raw = i % 2 ? uni(-25.0, 25.0) : uni(-7.0, 7.0);
    const double w = wrap_pi(raw);
    if (std::fabs(raw) > 2 * kPiD) ++beyond;
    CHECK(std::fabs(w) <= kPiD * (1 + 1e-15), "wrap left %.17g", w);
    CHECK(std::fabs(std::remainder(w - raw, 2 * kPiD)) < 1e-14, "wrap moved %.17g to %.17g", raw, w);
    if (std::fabs(raw) < kPiD) CHECK(w == raw, "wrap changed %.17g inside (-pi, pi) to %.17g", raw, w);
  }
  CHECK(beyond > 1000, "only %d angles beyond +-2 pi", beyond);
  CHECK(wrap_pi(0.0) == 0.0 && wrap_pi(-0.0) == 0.0, "wrap of a zero");
  CHECK(std::fabs(wrap_pi(kPiD)) == kPiD && std::fabs(wrap_pi(-kPiD)) == kPiD, "wrap of +-pi");
  CHECK(wrap_pi(2 * kPiD) == 0.0 && wrap_pi(-4 * kPiD) == 0.0, "wrap of whole turns");
  CHECK(std::isnan(wrap_pi(NAN)), "wrap of a NaN");
  std::printf("wrap: %d angles beyond 2 pi\n", beyond);
}

int main(int argc, char **argv) {
  check_wrap();
  if (argc > 2 && run_file(argv[1], argv[2])) return 1;
  if (g_fail) {
    std::printf("chain_jac_check: %d checks failed\n", g_fail);
    return 1;
  }
  std::printf("chain_jac_check ok\n");
  return 0;
}
