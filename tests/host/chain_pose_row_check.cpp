// chain_pose_row_check.cpp -- CPU check of csrc/ik_chain_pose_row.h, the row functions
// that chain_pose_kernel compiles: the chain with the tool frame and the joint axes,
// the two rotation errors, the 6-row solve with a lock mask and its active-set step.
// Stand-alone, built with AddressSanitizer + UndefinedBehaviorSanitizer by
// tests/test_chain_pose_cpu.py and run directly.
//
//   chain_pose_row_check          the built-in rows, then "chain_pose_row_check ok"
//   chain_pose_row_check IN OUT   also runs the file IN, raw float64: the number of
//       blocks, then per block nj, n, the DH table (4 nj: theta, d, a, alpha), jc (32:
//       ChainParams' layout), lo (8), hi (8), mask, lam2, w and n rows of theta[nj]
//       sin[nj] cos[nj] p[3] G[9].  Writes per row x y z, R (9, row-major), jx[nj] jy[nj]
//       jz[nj] wx[nj] wy[nj] wz[nj], e_w (3), er, delta[nj] (before the scaling), lock,
//       resolves, theta'[nj] (scaled, added and placed) to OUT; the test compares them
//       byte for byte with the numpy restatement.
//
// The rows are also checked by what they have to be, not by a copy of the chain: p and
// R are the translation and the rotation of the product of the nj 4 x 4 DH matrices
// Rz(theta) Tz(d) Tx(a) Rx(alpha), formed here in long double; axis i is z_{i-1} and
// linear column i is z_{i-1} x (p - o_{i-1}); and the position and the linear columns
// are chain_jac's own bits.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "ik_chain_pose_row.h"

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
  double lam2, w;
  const double *rows;
  int64_t n;
};

static double g_worst_p = 0.0, g_worst_r = 0.0, g_worst_w = 0.0, g_worst_j = 0.0;

static void worst(double e, double bound, double *acc, const char *what, int nj, long long r,
                  int i, int k) {
  *acc = e > *acc ? e : *acc;
  CHECK(e <= bound, "nj %d row %lld: %s[%d][%d] is %.3g off (bound %.3g)", nj, r, what, i, k, e,
        bound);
}

// One block's rows; out: 18 + 8 NJ doubles a row.  The bounds are chain_row_check.cpp's
// rule: 50 float64 roundings of a value of the chain's total length L = sum |a_i| +
// |d_i| for the effector and the linear columns, of 1 for R and the axes.
template <int NJ>
static void run_block(const Block &b, double *out) {
  double L = 0.0;
  for (int i = 0; i < NJ; ++i) L += std::fabs(b.dh[NJ + i]) + std::fabs(b.dh[2 * NJ + i]);
  const double bound1 = 50 * (DBL_EPSILON / 2), bound = bound1 * L;
  const int W = 18 + 8 * NJ;
  for (int64_t r = 0; r < b.n; ++r) {
    const double *th = b.rows + (3 * NJ + 12) * r, *s = th + NJ, *c = th + 2 * NJ,
                 *goal = th + 3 * NJ, *G = goal + 3;
    const PoseJacN<NJ> f = pose_jac<NJ>(b.P.jc, s, c);
    const ChainJacN<NJ> lin = chain_jac<NJ>(b.P.jc, s, c);
    CHECK(std::memcmp(&f.lin, &lin, sizeof(lin)) == 0, "row %lld: not chain_jac's bits",
          (long long)r);
    double *o = out + W * r;
    o[0] = f.lin.x, o[1] = f.lin.y, o[2] = f.lin.z;
    for (int i = 0; i < 3; ++i)
      for (int k = 0; k < 3; ++k) o[3 + 3 * i + k] = f.r[k][i];
    for (int k = 0; k < NJ; ++k) {
      o[12 + k] = f.lin.jx[k];
      o[12 + NJ + k] = f.lin.jy[k];
      o[12 + 2 * NJ + k] = f.lin.jz[k];
      o[12 + 3 * NJ + k] = f.wx[k];
      o[12 + 4 * NJ + k] = f.wy[k];
      o[12 + 5 * NJ + k] = f.wz[k];
    }
    CHECK(f.wx[0] == 0.0 && f.wy[0] == 0.0 && f.wz[0] == 1.0, "axis 1 is not (0, 0, 1)");
    double e[6], ew[3];
    e[0] = goal[0] - f.lin.x, e[1] = goal[1] - f.lin.y, e[2] = goal[2] - f.lin.z;
    pose_rot_step_error(f.r, G, ew);
    for (int k = 0; k < 3; ++k) {
      e[3 + k] = b.w * ew[k];
      o[12 + 6 * NJ + k] = ew[k];
    }
    o[15 + 6 * NJ] = pose_rot_error(f.r, G);
    double d[NJ];
    int rs = -1;
    const unsigned lock = pose_step<NJ>(f, e, b.w, b.lam2, th, b.P, d, &rs);
    CHECK(rs >= 0 && rs <= NJ && (lock & ~b.P.mask) == 0, "row %lld: lock %u resolves %d",
          (long long)r, lock, rs);
    if (!b.P.mask) {  // every joint free: the plain solve's bits
      double d0[NJ];
      pose_solve<NJ>(f, e, b.w, b.lam2, 0u, d0);
      CHECK(std::memcmp(d, d0, sizeof(d)) == 0 && lock == 0 && rs == 0, "free step != solve");
    }
    if (b.w == 0.0) {  // no rotation rows: chain_step's delta
      double d0[NJ];
      int rs0 = -1;
      const unsigned lock0 = chain_step<NJ>(f.lin, e[0], e[1], e[2], b.lam2, th, b.P, d0, &rs0);
      // (as numbers: a locked joint's delta is a sum of zero products, +0.0 or -0.0 by
      // the signs of q, and the three more terms here can turn a -0.0 into +0.0)
      bool eq = lock == lock0 && rs == rs0;
      for (int k = 0; k < NJ; ++k) eq = eq && d[k] == d0[k] && (d[k] != 0.0 || ((lock >> k) & 1u));
      CHECK(eq, "row %lld: w = 0 is not chain_step", (long long)r);
    }
    for (int k = 0; k < NJ; ++k) {
      o[16 + 6 * NJ + k] = d[k];
      if ((lock >> k) & 1u) CHECK(d[k] == 0.0, "row %lld: locked joint %d moves", (long long)r, k);
    }
    o[16 + 7 * NJ] = (double)lock;
    o[17 + 7 * NJ] = (double)rs;
    chain_scale<NJ>(d, 0.5);
    for (int k = 0; k < NJ; ++k) {
      const double t1 = chain_place<true>(th[k] + d[k], b.P, k);
      o[18 + 7 * NJ + k] = t1;
      if ((b.P.mask >> k) & 1u)
        CHECK(b.P.lo[k] <= t1 && t1 <= b.P.hi[k], "row %lld: joint %d left its limits",
              (long long)r, k);
    }
    // what the chain has to be
    M4 T[kChainMaxJoints + 1];
    frames_ld(NJ, b.dh, th, T);
    const ld p[3] = {T[NJ].m[0][3], T[NJ].m[1][3], T[NJ].m[2][3]};
    for (int k = 0; k < 3; ++k) {
      worst(std::fabs((double)((ld)o[k] - p[k])), bound, &g_worst_p, "effector", NJ, r, 0, k);
      for (int i = 0; i < 3; ++i)
        worst(std::fabs((double)((ld)f.r[k][i] - T[NJ].m[i][k])), bound1, &g_worst_r, "R", NJ, r, i,
              k);
    }
    for (int i = 0; i < NJ; ++i) {
      const ld z[3] = {T[i].m[0][2], T[i].m[1][2], T[i].m[2][2]};
      const ld v[3] = {p[0] - T[i].m[0][3], p[1] - T[i].m[1][3], p[2] - T[i].m[2][3]};
      const ld want[3] = {z[1] * v[2] - z[2] * v[1], z[2] * v[0] - z[0] * v[2],
                          z[0] * v[1] - z[1] * v[0]};
      const double got[3] = {f.lin.jx[i], f.lin.jy[i], f.lin.jz[i]};
      const double ax[3] = {f.wx[i], f.wy[i], f.wz[i]};
      for (int k = 0; k < 3; ++k) {
        worst(std::fabs((double)((ld)got[k] - want[k])), bound, &g_worst_j, "J", NJ, r, k, i);
        worst(std::fabs((double)((ld)ax[k] - z[k])), bound1, &g_worst_w, "axis", NJ, r, k, i);
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
    const size_t head = 2 + 4 * (size_t)nj + 32 + 8 + 8 + 3, roww = 3 * (size_t)nj + 12;
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
    b.w = q[50];
    b.rows = &v[at + head];
    b.n = n;
    const size_t base = out.size();
    out.resize(base + (18 + 8 * (size_t)nj) * (size_t)n);
    run_any(nj, b, out.data() + base);
    at += head + roww * (size_t)n;
    total += n;
  }
  if (at != v.size())
    return std::printf("%s: %zu doubles, the blocks end at %zu\n", in, v.size(), at), 1;
  std::FILE *f = std::fopen(outp, "wb");
  if (!f || std::fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) {
    std::printf("cannot write %s\n", outp);
    return 1;
  }
  std::fclose(f);
  std::printf("rows %lld: worst |effector - long double| %.3e, |R - long double| %.3e, |axis - "
              "z| %.3e, |J - geometric| %.3e\n", total, g_worst_p, g_worst_r, g_worst_w, g_worst_j);
  return 0;
}

// Rows whose outcome is known.
static void builtin_rows() {
  // the identity against itself: both errors zero; against a turn of pi about z the
  // step's error is zero too, the chord is 2
  const double I3[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  const double same[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, turned[9] = {-1, 0, 0, 0, -1, 0, 0, 0, 1};
  double ew[3];
  pose_rot_step_error(I3, same, ew);
  CHECK(ew[0] == 0.0 && ew[1] == 0.0 && ew[2] == 0.0 && pose_rot_error(I3, same) == 0.0,
        "the identity against itself");
  pose_rot_step_error(I3, turned, ew);
  CHECK(ew[0] == 0.0 && ew[1] == 0.0 && ew[2] == 0.0 && pose_rot_error(I3, turned) == 2.0,
        "a turn of pi: e_w (%g %g %g), er %g", ew[0], ew[1], ew[2], pose_rot_error(I3, turned));
  // a quarter turn about z: e_w = (0, 0, 1), er = 2 sin(pi / 4)
  const double quarter[9] = {0, -1, 0, 1, 0, 0, 0, 0, 1};
  pose_rot_step_error(I3, quarter, ew);
  CHECK(ew[0] == 0.0 && ew[1] == 0.0 && ew[2] == 1.0 && pose_rot_error(I3, quarter) == sqrt(2.0),
        "a quarter turn: e_w (%g %g %g), er %.17g", ew[0], ew[1], ew[2],
        pose_rot_error(I3, quarter));
  // every joint locked: A = lam2 I, delta all zero
  {
    ChainParams Q;
    std::memset(&Q, 0, sizeof(Q));
    for (int i = 0; i < 8; ++i) Q.lo[i] = -INFINITY, Q.hi[i] = INFINITY;
    for (int i = 0; i < 3; ++i) Q.lo[i] = Q.hi[i] = 0.0;
    Q.mask = 7u;
    PoseJacN<3> f = {};
    const ChainJacN<3> lin = {1.0, 2.0, 3.0, {-0.3, 0.7, 0.5}, {1.9, 0.1, 0.08}, {0.0, -1.2, -0.9}};
    f.lin = lin;
    f.wz[0] = 1.0, f.wx[1] = 0.6, f.wz[1] = 0.8, f.wy[2] = 1.0;
    const double t[3] = {0.0, 0.0, 0.0}, e[6] = {0.01, -0.02, 0.015, 0.1, -0.2, 0.3};
    double d[3];
    int rs = -1;
    const unsigned lock = pose_step<3>(f, e, 1.0, 1e-6, t, Q, d, &rs);
    CHECK(lock == 7u && rs >= 1 && rs <= 3 && d[0] == 0.0 && d[1] == 0.0 && d[2] == 0.0,
          "all fixed: lock %u resolves %d", lock, rs);
  }
}

int main(int argc, char **argv) {
  builtin_rows();
  if (argc > 2 && run_file(argv[1], argv[2])) return 1;
  if (g_fail) {
    std::printf("chain_pose_row_check: %d checks failed\n", g_fail);
    return 1;
  }
  std::printf("chain_pose_row_check ok\n");
  return 0;
}
