// ik_chain_pose.hip -- ik_chain_pose_solve: ik_chain_solve for a tool pose, position and
// orientation in one damped least-squares step, for any DH chain of 2..8 revolute
// joints (include/ikhip.h "Chain pose solve"; DESIGN.md section 3 "Chain pose solve").
//
// chain_pose_kernel<NJ, kLimited> is ik_chain.hip's kernel with six rows where that has
// three: one goal per lane, fp64 VALU, everything in registers, the joint loops fully
// unrolled, the table's constants and the limits in one by-value struct.  The row
// functions are ik_chain_pose_row.h (compiled by a host program too;
// kinematics/chain.py restates them); the scaling, the placing, the locks and the
// start points are ik_chain_row.h's, so with rot_weight = 0 and rot_tol = +inf the
// angles, steps, attempts and errors are ik_chain_solve's bit for bit.
//
// An attempt stops on the two errors the row reports, |p - x| and the chord
// sqrt(1/2 |R - G|_F^2), never on the step's own rotation error, which vanishes at a
// turn of pi.  Restarts are per lane as in ik_chain.hip, with the same known cost:
// converged lanes idle until their wave's slowest row ends.  The 6 x NJ matrix and the
// 6 x 6 factor fill the register file: 256 threads a block, one wave per SIMD from
// NJ = 6 (DESIGN.md has the table).  HBM per row: 96 B goal + 8 NJ B seed in, 8 NJ B
// angles (+ 4 B steps + 4 B attempt + 16 B errors) out, every access 8 bytes.
#include "ik_chain_pose.h"
#include "ik_chain_pose_row.h"
#include "ik_fk_chain.h"
#include "ik_launch.h"
#include "ik_stats.h"

namespace ikhip {

constexpr double kPoseClamp = 0.5;  // largest |delta_i| of one step, radians

template <int NJ, bool kLimited>
__global__ __launch_bounds__(256) void chain_pose_kernel(
    ChainParams P, ChainHome home, const double *pts, const double *rot, const double *seed,
    int64_t n, double tol, double rot_tol, double w, int max_iter, double lam2, int restarts,
    double *ang, int32_t *iters, int32_t *tries, double *fk_err, double *rot_err, DevStats *S) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool valid = i < n;
  double px = 0.0, py = 0.0, pz = 0.0, G[9], t[NJ], best[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) t[j] = 0.0;
#pragma unroll
  for (int j = 0; j < 9; ++j) G[j] = 0.0;
  if (valid) {
    px = pts[3 * i];
    py = pts[3 * i + 1];
    pz = pts[3 * i + 2];
#pragma unroll
    for (int j = 0; j < 9; ++j) G[j] = rot[9 * i + j];
#pragma unroll
    for (int j = 0; j < NJ; ++j)  // the seed (or the home pose), wrapped and projected
      t[j] = chain_place<kLimited>(seed ? seed[NJ * i + j] : home.th[j], P, j);
  }
#pragma unroll
  for (int j = 0; j < NJ; ++j) best[j] = t[j];
  const bool alpha_ok = !P.alpha_bad;  // some |alpha_i| > 2 pi: FK raises, the errors are NaN

  bool active = valid;
  int it = 0, tot = 0;      // steps of this attempt, of all attempts
  int a = 0, best_try = 0;  // this attempt, the attempt `best` holds
  double ep = 0.0, er = 0.0, best_ep = 0.0, best_er = 0.0, best_score = 0.0;
  for (;;) {
    double s[NJ], c[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) sincos_fk(t[j], &s[j], &c[j]);
    const PoseJacN<NJ> f = pose_jac<NJ>(P.jc, s, c);

    double e[6];
    e[0] = px - f.lin.x, e[1] = py - f.lin.y, e[2] = pz - f.lin.z;
    const double en = sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
    const double rn = pose_rot_error(f.r, G);
    bool fresh = false;  // t is a new start point: f is not its chain, no step this round
    if (active) {
      ep = alpha_ok ? en : __builtin_nan("");
      er = alpha_ok ? rn : __builtin_nan("");
      const bool isnan = ep != ep || er != er;
      const bool above = ep > tol || er > rot_tol;
      if (!above || isnan || it == max_iter) {  // the attempt ends
        const double score = ep + w * er;
        if (a == 0 || score < best_score) {  // the smallest score, the earliest on a tie
          best_score = score;
          best_ep = ep;
          best_er = er;
          best_try = a;
#pragma unroll
          for (int j = 0; j < NJ; ++j) best[j] = t[j];
        }
        if (above && !isnan && a < restarts) {
          ++a;
          it = 0;
          fresh = true;
#pragma unroll
          for (int j = 0; j < NJ; ++j)
            t[j] = chain_place<kLimited>(chain_start<kLimited>((uint64_t)i, (unsigned)a, j, P),
                                         P, j);
        } else {
          active = false;
        }
      }
    }
    if (!__any(active)) break;

    // e' = (e, w e_w); delta = J'^T (J' J'^T + lambda^2 I)^-1 e' (ik_chain_pose_row.h):
    // every column, or under joint limits without those the active-set loop locks
    double ew[3], d[NJ];
    pose_rot_step_error(f.r, G, ew);
#pragma unroll
    for (int k = 0; k < 3; ++k) e[3 + k] = w * ew[k];
    if constexpr (kLimited) {
      pose_step<NJ>(f, e, w, lam2, t, P, d, nullptr);
    } else {
      pose_solve<NJ>(f, e, w, lam2, 0u, d);
    }
    chain_scale<NJ>(d, kPoseClamp);
    if (active && !fresh) {
#pragma unroll
      for (int j = 0; j < NJ; ++j) t[j] = chain_place<kLimited>(t[j] + d[j], P, j);
      ++it;
      ++tot;
    }
  }

  if (valid) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) ang[NJ * i + j] = best[j];
    if (iters) iters[i] = tot;
    if (tries) tries[i] = best_try;
    if (fk_err) fk_err[i] = best_ep;
    if (rot_err) rot_err[i] = best_er;
  }
  // n_capped: rows that did not converge (a NaN error included); first_err: the lowest
  // of them with both errors finite; the fk sums are over the finite position errors
  const bool capped = valid && !(best_ep <= tol && best_er <= rot_tol);
  const bool pfinite = valid && best_ep <= 1.7976931348623157e308;  // (not NaN)
  const bool finite = pfinite && best_er <= 1.7976931348623157e308;
  if (capped && finite) record_error(S, i, IK_E_OUT_OF_REACH);
  block_iter_stats_acc(S, valid ? (unsigned long long)tot : 0ull, capped ? 1ull : 0ull,
                       valid ? tot : 0);
  const double fe = pfinite ? best_ep : 0.0;
  wave_fk_stats(S, fe, fe);
}

template <int NJ>
static void launch_pose_nj(const ChainParams &P, const ChainHome &home, const double *pts,
                           const double *rot, const double *seed, int64_t n, double tol,
                           double rot_tol, double rot_weight, int max_iter, double damping,
                           int restarts, double *ang, int32_t *iters, int32_t *tries,
                           double *fk_err, double *rot_err, DevStats *S, hipStream_t st) {
  const unsigned grid = (unsigned)((n + 255) / 256);
  // every joint free: the kernel without the limits' code
  if (P.mask) {
    kt_begin("chain_pose_limited_kernel", st);
    IK_LAUNCH((chain_pose_kernel<NJ, true>), dim3(grid), dim3(256), 0, st, P, home, pts, rot, seed,
              n, tol, rot_tol, rot_weight, max_iter, damping * damping, restarts, ang, iters, tries,
              fk_err, rot_err, S);
  } else {
    kt_begin("chain_pose_kernel", st);
    IK_LAUNCH((chain_pose_kernel<NJ, false>), dim3(grid), dim3(256), 0, st, P, home, pts, rot,
              seed, n, tol, rot_tol, rot_weight, max_iter, damping * damping, restarts, ang, iters,
              tries, fk_err, rot_err, S);
  }
  kt_end(st);
}

void launch_chain_pose_solve(int nj, const ChainParams &P, const ChainHome &home,
                             const double *pts, const double *rot, const double *seed, int64_t n,
                             double tol, double rot_tol, double rot_weight, int max_iter,
                             double damping, int restarts, double *ang, int32_t *iters,
                             int32_t *tries, double *fk_err, double *rot_err, DevStats *S,
                             hipStream_t st) {
  if (n <= 0) return;
#define IK_POSE_CASE(NJ)                                                                         \
  case NJ:                                                                                       \
    launch_pose_nj<NJ>(P, home, pts, rot, seed, n, tol, rot_tol, rot_weight, max_iter, damping,  \
                       restarts, ang, iters, tries, fk_err, rot_err, S, st);                     \
    break;
  switch (nj) {
    IK_POSE_CASE(2)
    IK_POSE_CASE(3)
    IK_POSE_CASE(4)
    IK_POSE_CASE(5)
    IK_POSE_CASE(6)
    IK_POSE_CASE(7)
    IK_POSE_CASE(8)
    default:
      break;  // (ik_chain_pose_solve refuses other lengths)
  }
#undef IK_POSE_CASE
}

}  // namespace ikhip
