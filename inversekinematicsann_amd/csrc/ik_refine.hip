// ik_refine.hip -- damped-least-squares polish of seed angles (ik_refine,
// ik_ann_solve_refined; DESIGN.md section 3 "Refine").
//
// One goal per lane, fp64 VALU, everything in registers.  Per step: the FK chain
// with its four Jacobian columns (ik_chain_jac.h, shared with the training loss's FK
// term), A = J J^T + lambda^2 I (3 x 3, six entries), LDL^T without pivoting,
// delta = J^T A^-1 e, the 0.5 rad clamp and the wrap to [-pi, pi] (ik_row.h).
// kinematics/refine.py restates it operation for operation; the only difference is
// sincos_fk against libm's sin / cos (<= 1.2e-16).
//
// The chain and the 3 x 3 solve (ik_refine_step.h) are compiled by host programs too.  With
// joint limits (ik_set_joint_limits) a second instantiation of the same kernel runs:
// the same chain, the step from that header's active-set loop (wave-uniform, the
// locked columns selected to +0.0), a limited joint clipped to [lo, hi] where a free
// one is wrapped.  Limits that never bind give the free instantiation's bits.
//
// The wave iterates until no lane is active; a finished lane keeps its angles (the
// update is a select) and recomputes the same error.  HBM per row: 24 B goal +
// 32 / 16 B seed in, 32 B angles (+ 4 B count + 8 B error) out.
#include "ik_fk_chain.h"
#include "ik_launch.h"
#include "ik_refine.h"
#include "ik_refine_step.h"
#include "ik_stats.h"

namespace ikhip {

constexpr double kRefineClamp = 0.5;  // largest |delta_i| of one step, radians

// kLimited: the robot's joint limits jl hold (wave-uniform, by value); a limited
// joint's angle is pulled into [lo, hi] where a free one is wrapped, and the step
// comes from the active-set loop.  Without, jl is not read.
template <typename SeedT, bool kLimited>
__global__ __launch_bounds__(256) void refine_kernel(const RobotConstDev *rc, const double *pts,
                                                     const SeedT *seed, int64_t n, double tol,
                                                     int max_iter, double lam2, double *ang,
                                                     int32_t *iters, double *fk_err,
                                                     int check_limits, DevStats *S,
                                                     JointLimits jl) {
  const RcConst k = (RcConst)rc;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool valid = i < n;
  double px = 0.0, py = 0.0, pz = 0.0, t0 = 0.0, t1 = 0.0, t2 = 0.0, t3 = 0.0;
  if (valid) {
    px = pts[3 * i];
    py = pts[3 * i + 1];
    pz = pts[3 * i + 2];
    t0 = wrap_pi((double)seed[4 * i]);
    t1 = wrap_pi((double)seed[4 * i + 1]);
    t2 = wrap_pi((double)seed[4 * i + 2]);
    t3 = wrap_pi((double)seed[4 * i + 3]);
    if constexpr (kLimited) {  // the projection of the seed
      t0 = (jl.mask & 1u) ? refine_project(t0, jl.lo[0], jl.hi[0]) : t0;
      t1 = (jl.mask & 2u) ? refine_project(t1, jl.lo[1], jl.hi[1]) : t1;
      t2 = (jl.mask & 4u) ? refine_project(t2, jl.lo[2], jl.hi[2]) : t2;
      t3 = (jl.mask & 8u) ? refine_project(t3, jl.lo[3], jl.hi[3]) : t3;
    }
    if (check_limits) {
      const double lim[6] = {k->lim[0], k->lim[1], k->lim[2], k->lim[3], k->lim[4], k->lim[5]};
      if (outside(lim, px, py, pz)) atomicMin(&S->first_oob, (unsigned long long)i);
    }
  }
  double jc[14];  // fk_trip_consts' per-joint constants, wave-uniform
#pragma unroll
  for (int j = 0; j < 14; ++j) jc[j] = k->jc[j];
  const bool alpha_ok = !k->alpha_bad;  // some |alpha_i| > 2 pi: FK raises, the error is NaN

  bool active = valid;
  int it = 0;
  double err = 0.0;
  for (;;) {
    double s[4], c[4];
    sincos_fk(t0, &s[0], &c[0]);
    sincos_fk(t1, &s[1], &c[1]);
    sincos_fk(t2, &s[2], &c[2]);
    sincos_fk(t3, &s[3], &c[3]);
    const ChainJac f = fk_chain_jac(jc, s, c);  // the effector and dFK / dtheta

    const double ex = px - f.x, ey = py - f.y, ez = pz - f.z;
    const double en = sqrt(ex * ex + ey * ey + ez * ez);
    if (active) {
      err = alpha_ok ? en : __builtin_nan("");
      if (!(err > tol) || it == max_iter) active = false;
    }
    if (!__any(active)) break;

    // delta = J'^T (J' J'^T + lambda^2 I)^-1 e (ik_refine_step.h): every column, or
    // under joint limits without those the active-set loop locks
    double dl[4];
    if constexpr (kLimited) {
      const double tt[4] = {t0, t1, t2, t3};
      refine_step(f.J, ex, ey, ez, lam2, tt, jl, dl, nullptr);
    } else {
      refine_solve(f.J, ex, ey, ez, lam2, 0u, dl);
    }
    double e0 = dl[0], e1 = dl[1], e2 = dl[2], e3 = dl[3];
    const double m = fmax(fmax(fabs(e0), fabs(e1)), fmax(fabs(e2), fabs(e3)));
    if (m > kRefineClamp) {
      const double sc = kRefineClamp / m;
      e0 = e0 * sc;
      e1 = e1 * sc;
      e2 = e2 * sc;
      e3 = e3 * sc;
    }
    if (active) {
      if constexpr (kLimited) {
        t0 = (jl.mask & 1u) ? refine_project(t0 + e0, jl.lo[0], jl.hi[0]) : wrap_pi(t0 + e0);
        t1 = (jl.mask & 2u) ? refine_project(t1 + e1, jl.lo[1], jl.hi[1]) : wrap_pi(t1 + e1);
        t2 = (jl.mask & 4u) ? refine_project(t2 + e2, jl.lo[2], jl.hi[2]) : wrap_pi(t2 + e2);
        t3 = (jl.mask & 8u) ? refine_project(t3 + e3, jl.lo[3], jl.hi[3]) : wrap_pi(t3 + e3);
      } else {
        t0 = wrap_pi(t0 + e0);
        t1 = wrap_pi(t1 + e1);
        t2 = wrap_pi(t2 + e2);
        t3 = wrap_pi(t3 + e3);
      }
      ++it;
    }
  }

  if (valid) {
    double2 *o = reinterpret_cast<double2 *>(ang + 4 * i);
    o[0] = make_double2(t0, t1);
    o[1] = make_double2(t2, t3);
    if (iters) iters[i] = it;
    if (fk_err) fk_err[i] = err;
  }
  // n_capped: rows that did not converge (a NaN error included)
  block_iter_stats_acc(S, valid ? (unsigned long long)it : 0ull,
                       (valid && !(err <= tol)) ? 1ull : 0ull, valid ? it : 0);
  const double fe = (valid && err <= 1.7976931348623157e308) ? err : 0.0;  // finite (not NaN)
  wave_fk_stats(S, fe, fe);
}

template <typename SeedT>
static void launch_refine_t(const RobotConstDev *rc, const double *pts, const SeedT *seed,
                            int64_t n, double tol, int max_iter, double damping, double *ang,
                            int32_t *iters, double *fk_err, bool check_limits,
                            const JointLimits &jl, DevStats *S, hipStream_t st) {
  if (n <= 0) return;
  const unsigned grid = (unsigned)((n + 255) / 256);
  // every joint free: the kernel without the limits' code
  if (jl.mask) {
    kt_begin("refine_limited_kernel", st);
    IK_LAUNCH((refine_kernel<SeedT, true>), dim3(grid), dim3(256), 0, st, rc, pts, seed, n, tol,
              max_iter, damping * damping, ang, iters, fk_err, check_limits ? 1 : 0, S, jl);
  } else {
    kt_begin("refine_kernel", st);
    IK_LAUNCH((refine_kernel<SeedT, false>), dim3(grid), dim3(256), 0, st, rc, pts, seed, n, tol,
              max_iter, damping * damping, ang, iters, fk_err, check_limits ? 1 : 0, S, jl);
  }
  kt_end(st);
}

void launch_refine(const RobotConstDev *rc, const double *pts, const double *seed, int64_t n,
                   double tol, int max_iter, double damping, double *ang, int32_t *iters,
                   double *fk_err, bool check_limits, const JointLimits &jl, DevStats *S,
                   hipStream_t st) {
  launch_refine_t(rc, pts, seed, n, tol, max_iter, damping, ang, iters, fk_err, check_limits, jl,
                  S, st);
}

void launch_refine_f32(const RobotConstDev *rc, const double *pts, const float *seed, int64_t n,
                       double tol, int max_iter, double damping, double *ang, int32_t *iters,
                       double *fk_err, bool check_limits, const JointLimits &jl, DevStats *S,
                       hipStream_t st) {
  launch_refine_t(rc, pts, seed, n, tol, max_iter, damping, ang, iters, fk_err, check_limits, jl,
                  S, st);
}

// ik_check_joint_limits: a row violates when a limited joint's wrapped angle is not
// inside [lo, hi] (a NaN is not).  The lowest violating row goes to first_err with
// IK_E_ANGLE_RANGE, the rows' count to n_capped (one atomic per wave).
__global__ __launch_bounds__(256) void check_joint_limits_kernel(JointLimits jl, const double *ang,
                                                                 int64_t n, DevStats *S) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool bad = false;
  if (i < n) {
    const double2 *a = reinterpret_cast<const double2 *>(ang + 4 * i);
    const double2 a01 = a[0], a23 = a[1];
    const double w[4] = {wrap_pi(a01.x), wrap_pi(a01.y), wrap_pi(a23.x), wrap_pi(a23.y)};
#pragma unroll
    for (int j = 0; j < 4; ++j)
      bad = bad | (((jl.mask >> j) & 1u) && !(jl.lo[j] <= w[j] && w[j] <= jl.hi[j]));
    if (bad) record_error(S, i, IK_E_ANGLE_RANGE);
  }
  const unsigned long long c = (unsigned long long)__popcll(__ballot(bad));
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(&S->n_capped[blockIdx.x % kStatShards], c);
}

void launch_check_joint_limits(const JointLimits &jl, const double *ang, int64_t n, DevStats *S,
                               hipStream_t st) {
  if (n <= 0 || !jl.mask) return;  // every joint free: nothing violates
  const unsigned grid = (unsigned)((n + 255) / 256);
  kt_begin("check_joint_limits_kernel", st);
  IK_LAUNCH(check_joint_limits_kernel, dim3(grid), dim3(256), 0, st, jl, ang, n, S);
  kt_end(st);
}

}  // namespace ikhip
