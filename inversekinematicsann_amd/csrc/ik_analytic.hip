// ik_analytic.hip -- closed-form IK with tool pitch and elbow choice
// (ik_analytic_solve; DESIGN.md section 3 "Analytic").
//
// One goal per lane, fp64 VALU, no loop, everything in registers: the row
// arithmetic of ik_analytic_row.h, the workspace check and the FK round trip
// through the library's own chain (fk_error_cs with the robot's real cos alpha1)
// in one launch.  A failed row (no pitch reaches the goal) stores NaN and reports
// its index; the lanes around it are not affected (the infeasible / nearest path
// is one short branch whose both sides leave the row finite or NaN by design).
// HBM per row: 24 B goal (+ 8 B pitch) in, 32 B angles (+ 8 B pitch + 8 B error) out.
#include "ik_analytic.h"
#include "ik_analytic_row.h"
#include "ik_fk_chain.h"
#include "ik_launch.h"
#include "ik_stats.h"

namespace ikhip {

__global__ __launch_bounds__(256) void analytic_kernel(const RobotConstDev *rc, const double *pts,
                                                       const double *pitch, int64_t n, double b,
                                                       int nearest, double *ang, double *pitch_out,
                                                       double *fk_err, int check_limits,
                                                       DevStats *S) {
  const RcConst k = (RcConst)rc;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool valid = i < n;
  double px = 0.0, py = 0.0, pz = 0.0, ph = 0.0;
  if (valid) {
    px = pts[3 * i];
    py = pts[3 * i + 1];
    pz = pts[3 * i + 2];
    if (pitch) ph = pitch[i];
  }
  double jc[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) jc[j] = k->jc[j];
  // jc[4 i] = a_{i+1}, jc[1] = d1 (fk_trip_consts)
  const AnalyticRobot R = {jc[1], jc[0], jc[4], jc[8], jc[12]};
  const AnalyticRow o = analytic_row(R, px, py, pz, pitch != nullptr, ph, b, nearest != 0);

  // |FK(theta) - p| through the library's chain; every angle is in [-pi, pi]
  const double th[4] = {o.t1, o.t2, o.t3, o.t4};
  double c[4], s[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) sincos_fk(o.fail ? 0.0 : th[j], &s[j], &c[j]);
  const double en = fk_error_cs(jc, c, s, !k->alpha_bad, px, py, pz);
  const double err = o.fail ? __builtin_nan("") : en;

  bool oob = false;
  if (valid && check_limits) {
    const double lim[6] = {k->lim[0], k->lim[1], k->lim[2], k->lim[3], k->lim[4], k->lim[5]};
    oob = outside(lim, px, py, pz);
  }
  // The lowest lane of a wave holds its lowest index: at most one atomic per wave,
  // and none once the word holds a lower index (a plain read first: with a third of
  // the rows failing, 16 K atomics on one word tripled the kernel's time; a stale
  // read only costs the atomic it would have saved).
  const int lane = threadIdx.x & 63;
  const unsigned long long oob_m = __ballot(oob), fail_m = __ballot(valid && o.fail);
  if (oob_m && lane == __ffsll((long long)oob_m) - 1 &&
      (unsigned long long)i < __atomic_load_n(&S->first_oob, __ATOMIC_RELAXED))
    atomicMin(&S->first_oob, (unsigned long long)i);
  if (fail_m && lane == __ffsll((long long)fail_m) - 1 &&
      ((unsigned long long)i << 8) < __atomic_load_n(&S->first_err_key, __ATOMIC_RELAXED))
    record_error(S, i, IK_E_OUT_OF_REACH);

  if (valid) {
    double2 *out = reinterpret_cast<double2 *>(ang + 4 * i);
    out[0] = make_double2(o.t1, o.t2);
    out[1] = make_double2(o.t3, o.t4);
    if (pitch_out) pitch_out[i] = o.phi;
    if (fk_err) fk_err[i] = err;
  }
  // n_capped: rows whose pitch was moved; no iterations
  block_iter_stats_acc(S, 0ull, (valid && o.moved) ? 1ull : 0ull, 0);
  const double fe = (valid && err <= 1.7976931348623157e308) ? err : 0.0;  // finite (not NaN)
  wave_fk_stats(S, fe, fe);
}

void launch_analytic(const RobotConstDev *rc, const double *pts, const double *pitch, int64_t n,
                     int elbow, bool nearest, double *ang, double *pitch_out, double *fk_err,
                     bool check_limits, DevStats *S, hipStream_t st) {
  if (n <= 0) return;
  const unsigned grid = (unsigned)((n + 255) / 256);
  kt_begin("analytic_kernel", st);
  IK_LAUNCH(analytic_kernel, dim3(grid), dim3(256), 0, st, rc, pts, pitch, n, (double)elbow,
            nearest ? 1 : 0, ang, pitch_out, fk_err, check_limits ? 1 : 0, S);
  kt_end(st);
}

}  // namespace ikhip
