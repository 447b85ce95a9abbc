// train_fk_row_check.cpp -- CPU check of the training loss's forward-kinematics term:
// the row function of csrc/ik_train_fk_row.h (the one the kernel compiles, here with
// libm's sines and cosines) and the new host arithmetic of csrc/ik_train_plan.cpp
// (the refusals of ik_ann_train_set_loss, dZ's factors, the weighted total, the
// epoch's fk means).  Stand-alone, built with -fsanitize=address,undefined by
// tests/test_train_fk_cpu.py and run directly.
//
// The row is checked by what it has to be, not by a copy of its chain: the effector
// is the translation of the product of the four 4 x 4 DH matrices
// Rz(theta) Tz(d) Tx(a) Rx(alpha), formed here in long double, and J_j . e is the
// derivative of F(theta) = |FK(theta) - p|^2 / 2, taken by central differences of
// that long double F.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "ik_train_fk_row.h"
#include "ik_train_plan.h"

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
// rows of dh: theta (not read), d, a, alpha
static void fk_ld(const double *dh, const ld th[4], ld out[3]) {
  M4 T = ident();
  for (int i = 0; i < 4; ++i) {
    M4 rz = ident(), tz = ident(), tx = ident(), rx = ident();
    rz.m[0][0] = cosl(th[i]), rz.m[0][1] = -sinl(th[i]);
    rz.m[1][0] = sinl(th[i]), rz.m[1][1] = cosl(th[i]);
    tz.m[2][3] = (ld)dh[4 + i];
    tx.m[0][3] = (ld)dh[8 + i];
    const ld al = (ld)dh[12 + i];
    rx.m[1][1] = cosl(al), rx.m[1][2] = -sinl(al);
    rx.m[2][1] = sinl(al), rx.m[2][2] = cosl(al);
    T = mul(T, mul(mul(mul(rz, tz), tx), rx));
  }
  out[0] = T.m[0][3], out[1] = T.m[1][3], out[2] = T.m[2][3];
}
static ld half_sq(const double *dh, const ld th[4], const ld p[3]) {
  ld f[3];
  fk_ld(dh, th, f);
  ld s = 0.0L;
  for (int k = 0; k < 3; ++k) s += (f[k] - p[k]) * (f[k] - p[k]);
  return s / 2;
}

static const double kPiD = 3.141592653589793;
static const double kTables[][16] = {
    // SixDOFRobot's, tests/robots.py GEN_A and GEN_B, tests/test_refine_cpu.py SKEW_DH
    {0.0, kPiD / 2, 0.0, 0.0, 2.0, 0.0, 0.0, 0.0, 0.0, 2.0, 2.0, 2.0, kPiD / 2, 0.0, 0.0, 0.0},
    {0.0, 1.1, -0.5, 0.3, 1.5, 0.25, -0.2, 0.15, 0.3, 1.7, 2.3, 0.9, 1.4, -0.4, 0.35, 1.2},
    {0.0, 0.9, 0.4, -0.6, 1.8, 0.3, -0.25, 0.2, 0.25, 1.9, 2.1, 1.6, 1.3, 0.5, -0.3, 0.7},
    {0.0, kPiD / 2, 0.0, 0.0, 2.0, 0.0, 0.3, 0.0, 0.0, 2.0, 2.0, 2.0, kPiD / 2, 0.4, 0.0, 0.0},
};

static void consts_of(const double *dh, double jc[16]) {
  for (int i = 0; i < 4; ++i) {
    jc[4 * i + 0] = dh[8 + i], jc[4 * i + 1] = dh[4 + i];
    jc[4 * i + 2] = std::cos(dh[12 + i]), jc[4 * i + 3] = std::sin(dh[12 + i]);
  }
}

// The row against long double.  Bounds: FK's entries are at most the chain's total
// length, ~9 here, and the goals lie within ~10 of them, so |e| <~ 20, e . e <~ 400 and
// |J_j . e| <~ 200.  The float64 row rounds each of its ~100 operations to 1.1e-16
// relative of values of that size: 1e-12 absolute is 50 x that.  The central
// difference of F with h = 2^-20 has truncation h^2 / 6 |F'''| <~ 1.5e-13 * 3e3 and
// long double rounding 5.4e-20 * 400 / h = 2e-11: 1e-9 absolute covers both.
static void check_rows() {
  uint64_t x = 88172645463325252ull;
  auto uni = [&](double lo, double hi) {
    x ^= x << 13, x ^= x >> 7, x ^= x << 17;  // xorshift64
    return lo + (double)(x >> 11) * 0x1p-53 * (hi - lo);
  };
  const TrainFkScale sc = {{2.5, 0.3, 1.5}, {1.2, 1.8, 1.4}, {0.2, 0.8, -0.7, 0.1},
                           {0.9, 0.5, 0.6, 0.8}};
  double worst_ee = 0.0, worst_je = 0.0;
  int wrapped = 0;
  for (const auto &dh : kTables) {
    double jc[16];
    consts_of(dh, jc);
    for (int row = 0; row < 200; ++row) {
      float a[4], xin[3];
      // every fourth row: angles beyond +-2 pi, where only the wrap keeps sincos valid
      const double span = row % 4 == 3 ? 12.0 : 3.0;
      for (int j = 0; j < 4; ++j) a[j] = (float)uni(-span, span);
      for (int k = 0; k < 3; ++k) xin[k] = (float)uni(-2.0, 2.0);
      double th[4], s[4], c[4];
      train_fk_angles(sc, a, th);
      ld thl[4], p[3];
      for (int j = 0; j < 4; ++j) {
        const double raw = (double)a[j] * sc.ys[j] + sc.ym[j];
        if (std::fabs(raw) > 2 * kPiD) ++wrapped;
        CHECK(std::fabs(th[j]) <= kPiD * (1 + 1e-15), "wrap left %.17g", th[j]);
        CHECK(std::fabs(std::remainder(th[j] - raw, 2 * kPiD)) < 1e-14, "wrap moved %.17g to %.17g",
              raw, th[j]);
        s[j] = std::sin(th[j]), c[j] = std::cos(th[j]);
        thl[j] = (ld)raw;  // FK is periodic: the unwrapped angle, in long double
      }
      for (int k = 0; k < 3; ++k) p[k] = (ld)((double)xin[k] * sc.xs[k] + sc.xm[k]);
      const TrainFkRow o = train_fk_row(jc, sc, s, c, xin, true);
      const ld f0 = half_sq(dh, thl, p);
      const double dee = std::fabs((double)((ld)o.ee - 2 * f0));
      worst_ee = dee > worst_ee ? dee : worst_ee;
      CHECK(dee <= 1e-12, "e . e %.17g, long double %.17Lg", o.ee, 2 * f0);
      const ld h = 0x1p-20L;
      for (int j = 0; j < 4; ++j) {
        ld tp[4] = {thl[0], thl[1], thl[2], thl[3]}, tm[4] = {thl[0], thl[1], thl[2], thl[3]};
        tp[j] += h, tm[j] -= h;
        const ld want = (half_sq(dh, tp, p) - half_sq(dh, tm, p)) / (2 * h);
        const double dje = std::fabs((double)((ld)o.je[j] - want));
        worst_je = dje > worst_je ? dje : worst_je;
        CHECK(dje <= 1e-9, "J_%d . e %.17g, central difference %.17Lg", j, o.je[j], want);
      }
      if (row == 0) {
        const TrainFkRow bad = train_fk_row(jc, sc, s, c, xin, false);
        CHECK(std::isnan(bad.ee) && std::isnan(bad.je[0]) && std::isnan(bad.je[3]),
              "alpha_bad row: %g %g", bad.ee, bad.je[0]);
      }
    }
  }
  CHECK(wrapped > 100, "only %d angles beyond +-2 pi", wrapped);
  std::printf("rows: worst |e.e - long double| %.3e, worst |J.e - central difference| %.3e, "
              "%d angles beyond 2 pi\n", worst_ee, worst_je, wrapped);
}

// ---- the plan's new functions ----------------------------------------------------
static void check_epoch_fk() {
  long cases = 0;
  for (int64_t nt = 1; nt <= 40; ++nt)
    for (int batch = 1; batch <= 9; ++batch)
      for (int64_t nv : {0, 1, 8, 19}) {
        const TrainEpoch e = train_epoch(nt, nv, batch, 8);
        // every slot's sum is rows * c: both means are c
        std::vector<double> sums;
        for (int64_t s = 0; s < e.steps; ++s) sums.push_back(e.step_rows(s) * 1.7);
        for (int64_t v = 0; v < e.vchunks; ++v) sums.push_back(e.chunk_rows(v) * 1.7);
        double tf = -1.0, vf = -1.0;
        train_epoch_fk(e, sums.data(), &tf, &vf);
        CHECK(std::fabs(tf - 1.7) <= (2.0 * e.steps + 8.0) * DBL_EPSILON * 1.7,
              "%lld by %d: constant fk came out %.17g", (long long)nt, batch, tf);
        if (nv == 0)
          CHECK(std::isnan(vf), "no validation rows: val fk %g", vf);
        else
          CHECK(std::fabs(vf - 1.7) <= (2.0 * e.vchunks + 8.0) * DBL_EPSILON * 1.7,
                "%lld validation rows: constant fk came out %.17g", (long long)nv, vf);
        ++cases;
      }
  CHECK(cases == 40 * 9 * 4, "the sweep ran %ld cases", cases);
  // ragged steps (13 rows by 5: 5, 5, 3; 19 validation rows by 8: 8, 8, 3) with unequal
  // sums: weighting the steps' means by their rows is sum(sums) / rows, which the
  // plain mean of the steps' means is not
  const TrainEpoch e = train_epoch(13, 19, 5, 8);
  const double sums[6] = {4.0, 11.0, 0.75, 2.5, 30.0, 1.25};
  double tf = -1.0, vf = -1.0;
  train_epoch_fk(e, sums, &tf, &vf);
  const ld want_t = (4.0L + 11.0L + 0.75L) / 13.0L, want_v = (2.5L + 30.0L + 1.25L) / 19.0L;
  CHECK(std::fabs((double)((ld)tf - want_t)) <= 1e-15 * (double)want_t, "ragged fk %.17g", tf);
  CHECK(std::fabs((double)((ld)vf - want_v)) <= 1e-15 * (double)want_v, "ragged val fk %.17g", vf);
  const double plain = (4.0 / 5 + 11.0 / 5 + 0.75 / 3) / 3;
  CHECK(std::fabs(plain - (double)want_t) > 1e-3, "a blunt case");
}

static void check_weights() {
  // (1, 0) is today's arithmetic, bit for bit
  for (int rows : {1, 3, 24, 32, 300, 1024, 4096})
    for (int dL : {1, 2, 4}) {
      const double was = 2.0 / ((double)rows * (double)dL);
      CHECK(train_dz_mse_factor(1.0, rows, dL) == was, "mse factor at %d x %d", rows, dL);
      CHECK(std::fabs(train_dz_mse_factor(0.25, rows, dL) - 0.25 * was) <= DBL_EPSILON * was,
            "weighted mse factor at %d x %d", rows, dL);
      CHECK(std::fabs(train_dz_fk_factor(3.0, rows) - 6.0 / rows) <= DBL_EPSILON * 6.0 / rows,
            "fk factor at %d", rows);
    }
  const double m = 0.40312345678912345;
  CHECK(train_total_loss(1.0, 0.0, m, std::nan("")) == m, "(1, 0) is the mse itself");
  CHECK(train_total_loss(2.0, 0.0, m, std::nan("")) == 2.0 * m, "(2, 0)");
  CHECK(std::isnan(train_total_loss(1.0, 0.0, std::nan(""), 3.0)), "a NaN mse");
  CHECK(train_total_loss(0.5, 2.0, m, 0.125) == 0.5 * m + 0.25, "(0.5, 2)");
  CHECK(train_total_loss(0.0, 1.0, m, 0.125) == 0.125, "(0, 1)");
  CHECK(std::isnan(train_total_loss(1.0, 0.25, m, std::nan(""))), "a NaN fk");
}

static void expect(const std::string &got, const char *want, const char *what) {
  CHECK(got == want, "%s: '%s', expected '%s'", what, got.c_str(), want);
}

static void check_refusals() {
  const double xm[3] = {2.5, 0.3, 1.5}, xs[3] = {1.2, 1.8, 1.4};
  const double ym[4] = {0.2, 0.8, -0.7, 0.1}, ys[4] = {0.9, 0.5, 0.6, 0.8};
  auto why = [&](bool begun, int d0, int dL, double wm, double wf, const double *a = nullptr,
                 const double *b = nullptr, const double *c = nullptr, const double *d = nullptr) {
    return train_set_loss_refusal(begun, d0, dL, wm, wf, a, b, c, d);
  };
  expect(why(true, 3, 4, 1.0, 0.25, xm, xs, ym, ys), "", "a plain set_loss");
  expect(why(true, 3, 4, 0.0, 1.0, xm, xs, ym, ys), "", "the fk term alone");
  expect(why(true, 5, 2, 1.0, 0.0), "", "(1, 0) without scalers, any widths");
  expect(why(true, 5, 2, 2.5, 0.0), "", "a weighted mse");
  expect(why(false, 3, 4, 1.0, 0.25, xm, xs, ym, ys), "before ik_ann_train_begin", "no state");
  expect(why(false, 0, 0, 1.0, 0.0), "before ik_ann_train_begin", "no state, (1, 0)");
  const char *bad_w = "the weights must be finite and not negative";
  for (double v : {-1.0, -0.0 - 1e-300, (double)NAN, (double)INFINITY, -(double)INFINITY}) {
    expect(why(true, 3, 4, v, 1.0, xm, xs, ym, ys), bad_w, "mse_weight");
    expect(why(true, 3, 4, 1.0, v, xm, xs, ym, ys), bad_w, "fk_weight");
  }
  expect(why(true, 3, 4, 0.0, 0.0, xm, xs, ym, ys), "both weights are 0", "(0, 0)");
  expect(why(true, 5, 4, 1.0, 0.5, xm, xs, ym, ys),
         "the fk term needs 3 inputs and 4 outputs, the network has 5 and 4", "5 inputs");
  expect(why(true, 3, 2, 1.0, 0.5, xm, xs, ym, ys),
         "the fk term needs 3 inputs and 4 outputs, the network has 3 and 2", "2 outputs");
  expect(why(true, 3, 4, 1.0, 0.5, nullptr, xs, ym, ys), "NULL scaler array", "x_mean NULL");
  expect(why(true, 3, 4, 1.0, 0.5, xm, nullptr, ym, ys), "NULL scaler array", "x_scale NULL");
  expect(why(true, 3, 4, 1.0, 0.5, xm, xs, nullptr, ys), "NULL scaler array", "y_mean NULL");
  expect(why(true, 3, 4, 1.0, 0.5, xm, xs, ym, nullptr), "NULL scaler array", "y_scale NULL");
  for (double v : {(double)NAN, (double)INFINITY}) {
    double a3[3] = {2.5, 0.3, v}, b3[3] = {1.2, v, 1.4}, c4[4] = {0.2, 0.8, -0.7, v},
           d4[4] = {v, 0.5, 0.6, 0.8};
    expect(why(true, 3, 4, 1.0, 0.5, a3, xs, ym, ys), "x_mean[2] is not finite", "x_mean");
    expect(why(true, 3, 4, 1.0, 0.5, xm, b3, ym, ys), "x_scale[1] is not finite", "x_scale");
    expect(why(true, 3, 4, 1.0, 0.5, xm, xs, c4, ys), "y_mean[3] is not finite", "y_mean");
    expect(why(true, 3, 4, 1.0, 0.5, xm, xs, ym, d4), "y_scale[0] is not finite", "y_scale");
  }
  double z3[3] = {1.2, 1.8, 0.0}, z4[4] = {0.9, -0.0, 0.6, 0.8}, m0[3] = {0.0, 0.0, 0.0};
  expect(why(true, 3, 4, 1.0, 0.5, xm, z3, ym, ys), "x_scale[2] is 0", "x_scale 0");
  expect(why(true, 3, 4, 1.0, 0.5, xm, xs, ym, z4), "y_scale[1] is 0", "y_scale -0");
  expect(why(true, 3, 4, 1.0, 0.5, m0, xs, ym, ys), "", "a mean of 0 is fine");
}

int main() {
  check_rows();
  check_epoch_fk();
  check_weights();
  check_refusals();
  if (g_fail) {
    std::printf("train_fk_row_check: %d checks failed\n", g_fail);
    return 1;
  }
  std::printf("train_fk_row_check ok\n");
  return 0;
}
