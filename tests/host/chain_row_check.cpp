// chain_row_check.cpp -- CPU check of csrc/ik_chain_row.h, the row functions that
// chain_solve_kernel compiles: the NJ-joint chain with its Jacobian, the solve with a
// lock mask, the active-set step, the scaling and placing, and the start-point hash.
// Stand-alone, built with AddressSanitizer + UndefinedBehaviorSanitizer by
// tests/test_chain_cpu.py and run directly.
//
//   chain_row_check            the built-in rows, then "chain_row_check ok"
//   chain_row_check IN OUT     also runs the file IN, raw float64: the number of blocks,
//       then per block nj, n, the DH table (4 nj: theta, d, a, alpha), jc (32:
//       ChainParams' layout), lo (8), hi (8), mask, lam2 and n rows of theta[nj]
//       sin[nj] cos[nj] goal[3]; then the number of hash triples h and h rows of
//       (row, attempt, joint).  Writes per row x y z, jx[nj] jy[nj] jz[nj], delta[nj]
//       (before the scaling), lock, resolves, theta'[nj] (scaled, added and placed), and
//       then the h uniform numbers, to OUT; the test compares them byte for byte with
//       the numpy restatement.
//
// The rows are also checked by what they have to be, not by a copy of the chain: the
// effector is the translation of the product of the nj 4 x 4 DH matrices
// Rz(theta) Tz(d) Tx(a) Rx(alpha), formed here in long double, and column i of the
// Jacobian is the geometric one of a revolute joint, z_{i-1} x (p - o_{i-1}).
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "ik_chain_row.h"

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
static void frames_ld(int nj, const double *dh, const double *th, M4 *T) {
  T[0] = ident();
  for (int i = 0; i < nj; ++i) {
    M4 rz = ident(), tz = ident(), tx = ident(), rx = ident();
    const ld t = (ld)th[i], al = (ld)dh[3 * nj + i];
    rz.m[0][0] = cosl(t), rz.m[0][1] = -sinl(t);
    rz.m[1][0] = sinl(t), rz.m[1][1] = cosl(t);
    tz.m[2][3] = (ld)dh[nj + i];
    tx.m[0][3] = (ld)dh[2 * nj + i];
    rx.m[1][1] = cosl(al), rx.m[1][2] = -sinl(al);
    rx.m[2][1] = sinl(al), rx.m[2][2] = cosl(al);
    T[i + 1] = mul(T[i], mul(mul(mul(rz, tz), tx), rx));
  }
}

struct Block {
  const double *dh;
  ChainParams P;
  double lam2;
  const double *rows;
  int64_t n;
};

static double g_worst_p = 0.0, g_worst_j = 0.0;

// One block's rows; out: 5 + 5 NJ doubles a row.  The bound is chain_jac_check.cpp's
// rule: 50 x one float64 rounding of a value of the chain's total length L = sum |a_i| +
// |d_i|, which bounds the effector's and the Jacobian's entries.
template <int NJ>
static void run_block(const Block &b, double *out) {
  double L = 0.0;
  for (int i = 0; i < NJ; ++i) L += std::fabs(b.dh[NJ + i]) + std::fabs(b.dh[2 * NJ + i]);
  const double bound = 50 * (DBL_EPSILON / 2) * L;
  const int W = 5 + 5 * NJ;
  for (int64_t r = 0; r < b.n; ++r) {
    const double *th = b.rows + (3 * NJ + 3) * r, *s = th + NJ, *c = th + 2 * NJ,
                 *goal = th + 3 * NJ;
    const ChainJacN<NJ> f = chain_jac<NJ>(b.P.jc, s, c);
    double *o = out + W * r;
    o[0] = f.x, o[1] = f.y, o[2] = f.z;
    for (int k = 0; k < NJ; ++k) {
      o[3 + k] = f.jx[k];
      o[3 + NJ + k] = f.jy[k];
      o[3 + 2 * NJ + k] = f.jz[k];
    }
    CHECK(f.jz[0] == 0.0 && !std::signbit(f.jz[0]), "column 1 has a z part");
    const double ex = goal[0] - f.x, ey = goal[1] - f.y, ez = goal[2] - f.z;
    double d[NJ];
    int rs = -1;
    const unsigned lock = chain_step<NJ>(f, ex, ey, ez, b.lam2, th, b.P, d, &rs);
    CHECK(rs >= 0 && rs <= NJ && (lock & ~b.P.mask) == 0, "row %lld: lock %u resolves %d",
          (long long)r, lock, rs);
    if (!b.P.mask) {  // every joint free: the plain solve's bits
      double d0[NJ];
      chain_solve<NJ>(f, ex, ey, ez, b.lam2, 0u, d0);
      CHECK(std::memcmp(d, d0, sizeof(d)) == 0 && lock == 0 && rs == 0, "free step != solve");
    }
    for (int k = 0; k < NJ; ++k) {
      o[3 + 3 * NJ + k] = d[k];
      if ((lock >> k) & 1u) CHECK(d[k] == 0.0, "row %lld: locked joint %d moves", (long long)r, k);
    }
    o[3 + 4 * NJ] = (double)lock;
    o[4 + 4 * NJ] = (double)rs;
    chain_scale<NJ>(d, 0.5);
    for (int k = 0; k < NJ; ++k) {
      CHECK(!(std::fabs(d[k]) > 0.5000000000000002), "row %lld: |delta| %g after the scaling",
            (long long)r, d[k]);
      const double t1 = chain_place<true>(th[k] + d[k], b.P, k);
      o[5 + 4 * NJ + k] = t1;
      if ((b.P.mask >> k) & 1u)
        CHECK(b.P.lo[k] <= t1 && t1 <= b.P.hi[k], "row %lld: joint %d left its limits",
              (long long)r, k);
    }
    // what the chain has to be
    M4 T[kChainMaxJoints + 1];
    frames_ld(NJ, b.dh, th, T);
    const ld p[3] = {T[NJ].m[0][3], T[NJ].m[1][3], T[NJ].m[2][3]};
    for (int k = 0; k < 3; ++k) {
      const double e = std::fabs((double)((ld)o[k] - p[k]));
      g_worst_p = e > g_worst_p ? e : g_worst_p;
      CHECK(e <= bound, "nj %d row %lld: effector[%d] %.17g, long double %.17Lg (bound %.3g)", NJ,
            (long long)r, k, o[k], p[k], bound);
    }
    for (int i = 0; i < NJ; ++i) {
      const ld z[3] = {T[i].m[0][2], T[i].m[1][2], T[i].m[2][2]};
      const ld v[3] = {p[0] - T[i].m[0][3], p[1] - T[i].m[1][3], p[2] - T[i].m[2][3]};
      const ld want[3] = {z[1] * v[2] - z[2] * v[1], z[2] * v[0] - z[0] * v[2],
                          z[0] * v[1] - z[1] * v[0]};
      const double got[3] = {f.jx[i], f.jy[i], f.jz[i]};
      if (i == 0) CHECK(want[2] == 0.0L, "column 1 has a z part: %.17Lg", want[2]);
      for (int k = 0; k < 3; ++k) {
        const double e = std::fabs((double)((ld)got[k] - want[k]));
        g_worst_j = e > g_worst_j ? e : g_worst_j;
        CHECK(e <= bound, "nj %d row %lld: J[%d][%d] %.17g, geometric %.17Lg (bound %.3g)", NJ,
              (long long)r, k, i, got[k], want[k], bound);
      }
    }
  }
}

static void run_any(int nj, const Block &b, double *out) {
  switch (nj) {
    case 2: run_block<2>(b, out); break;
    case 3: run_block<3>(b, out); break;
    case 4: run_block<4>(b, out); break;
    case 5: run_block<5>(b, out); break;
    case 6: run_block<6>(b, out); break;
    case 7: run_block<7>(b, out); break;
    case 8: run_block<8>(b, out); break;
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
  if (v.empty()) {
    std::printf("cannot read %s\n", in);
    return 1;
  }
  std::vector<double> out;
  size_t at = 1;
  long long total = 0;
  for (int t = 0; t < (int)v[0]; ++t) {
    if (at + 2 > v.size()) return std::printf("%s: block %d is cut short\n", in, t), 1;
    const int nj = (int)v[at];
    const int64_t n = (int64_t)v[at + 1];
    if (nj < kChainMinJoints || nj > kChainMaxJoints || n < 0)
      return std::printf("%s: block %d: nj %d n %lld\n", in, t, nj, (long long)n), 1;
    const size_t head = 2 + 4 * (size_t)nj + 32 + 8 + 8 + 2, roww = 3 * (size_t)nj + 3;
    if (at + head + roww * (size_t)n > v.size())
      return std::printf("%s: block %d is cut short\n", in, t), 1;
    Block b;
    b.dh = &v[at + 2];
    const double *q = b.dh + 4 * nj;
    std::memset(&b.P, 0, sizeof(b.P));
    for (int i = 0; i < 8; ++i)
      for (int k = 0; k < 4; ++k) b.P.jc[i][k] = q[4 * i + k];
    for (int i = 0; i < 8; ++i) {
      b.P.lo[i] = q[32 + i];
      b.P.hi[i] = q[40 + i];
    }
    b.P.mask = (unsigned)q[48];
    b.lam2 = q[49];
    b.rows = &v[at + head];
    b.n = n;
    const size_t base = out.size();
    out.resize(base + (5 + 5 * (size_t)nj) * (size_t)n);
    run_any(nj, b, out.data() + base);
    at += head + roww * (size_t)n;
    total += n;
  }
  if (at >= v.size()) return std::printf("%s: no hash block\n", in), 1;
  const size_t h = (size_t)v[at];
  if (at + 1 + 3 * h != v.size())
    return std::printf("%s: %zu doubles, the blocks end at %zu\n", in, v.size(), at + 1 + 3 * h), 1;
  for (size_t k = 0; k < h; ++k) {
    const double *tr = &v[at + 1 + 3 * k];
    const double u = chain_start_u((uint64_t)tr[0], (unsigned)tr[1], (unsigned)tr[2]);
    CHECK(u >= 0.0 && u < 1.0, "u = %.17g", u);
    out.push_back(u);
  }
  std::FILE *f = std::fopen(outp, "wb");
  if (!f || std::fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) {
    std::printf("cannot write %s\n", outp);
    return 1;
  }
  std::fclose(f);
  std::printf("rows %lld, hashes %zu: worst |effector - long double| %.3e, worst |J - geometric| "
              "%.3e\n", total, h, g_worst_p, g_worst_j);
  return 0;
}

// Rows whose outcome is known.
static void builtin_rows() {
  const double kInf = INFINITY, kPiD = 3.141592653589793;
  ChainParams P;
  std::memset(&P, 0, sizeof(P));
  for (int i = 0; i < 8; ++i) P.lo[i] = -kInf, P.hi[i] = kInf;
  // the placing: a free joint wrapped, a limited one clipped, a NaN kept
  P.lo[1] = -0.5, P.hi[1] = 0.25, P.mask = 2u;
  CHECK(chain_place<true>(7.0, P, 0) == wrap_pi(7.0) && chain_place<true>(7.0, P, 1) == 0.25 &&
            chain_place<true>(-7.0, P, 1) == -0.5 && chain_place<true>(0.1, P, 1) == 0.1,
        "chain_place under limits");
  CHECK(chain_place<false>(7.0, P, 1) == wrap_pi(7.0), "chain_place without limits");
  CHECK(std::isnan(chain_place<true>(NAN, P, 1)) && std::isnan(chain_place<true>(NAN, P, 0)),
        "chain_place(NaN)");
  // start points: inside [lo', hi'], the free interval is [-pi, pi]; distinct per (row, a, j)
  double lo_seen = 1.0, hi_seen = 0.0;
  for (uint64_t row = 0; row < 2000; ++row)
    for (unsigned a = 1; a < 4; ++a) {
      const double u = chain_start_u(row, a, 2), t0 = chain_start<true>(row, a, 0, P),
                   t1 = chain_start<true>(row, a, 1, P), tf = chain_start<false>(row, a, 1, P);
      lo_seen = u < lo_seen ? u : lo_seen;
      hi_seen = u > hi_seen ? u : hi_seen;
      CHECK(t0 >= -kPiD && t0 <= kPiD && tf >= -kPiD && tf <= kPiD, "a free start %g %g", t0, tf);
      CHECK(t1 >= -0.5 && t1 <= 0.25, "a limited start %g", t1);
      CHECK(chain_start_u(row, a, 0) != chain_start_u(row, a, 1) &&
                chain_start_u(row, a, 0) != chain_start_u(row, a + 1, 0) &&
                chain_start_u(row, a, 0) != chain_start_u(row + 1, a, 0),
            "equal start numbers at row %llu", (unsigned long long)row);
    }
  CHECK(lo_seen < 0.01 && hi_seen > 0.99, "start numbers span [%g, %g]", lo_seen, hi_seen);
  // every joint locked: A = lam2 I, delta all zero
  {
    ChainParams Q = P;
    for (int i = 0; i < 3; ++i) Q.lo[i] = Q.hi[i] = 0.0;
    Q.mask = 7u;
    ChainJacN<3> f = {1.0, 2.0, 3.0, {-0.3, 0.7, 0.5}, {1.9, 0.1, 0.08}, {0.0, -1.2, -0.9}};
    const double t[3] = {0.0, 0.0, 0.0};
    double d[3];
    int rs = -1;
    const unsigned lock = chain_step<3>(f, 0.01, -0.02, 0.015, 1e-6, t, Q, d, &rs);
    CHECK(lock == 7u && rs >= 1 && rs <= 3 && d[0] == 0.0 && d[1] == 0.0 && d[2] == 0.0,
          "all fixed: lock %u resolves %d", lock, rs);
  }
  // the scaling keeps the direction and caps the largest entry at the clamp
  {
    double d[3] = {0.2, -2.0, 1.0};
    chain_scale<3>(d, 0.5);
    CHECK(d[1] == -0.5 && d[0] == 0.2 * (0.5 / 2.0) && d[2] == 1.0 * (0.5 / 2.0), "chain_scale");
    double e[2] = {0.2, -0.5};
    chain_scale<2>(e, 0.5);
    CHECK(e[0] == 0.2 && e[1] == -0.5, "chain_scale at the clamp");
  }
}

int main(int argc, char **argv) {
  builtin_rows();
  if (argc > 2 && run_file(argv[1], argv[2])) return 1;
  if (g_fail) {
    std::printf("chain_row_check: %d checks failed\n", g_fail);
    return 1;
  }
  std::printf("chain_row_check ok\n");
  return 0;
}
