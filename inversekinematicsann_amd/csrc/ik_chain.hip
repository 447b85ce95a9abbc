// ik_chain.hip -- ik_chain_solve: damped least squares with joint limits and random
// restarts for any DH chain of 2..8 revolute joints (include/ikhip.h "Chain solve";
// DESIGN.md section 3 "Chain solve").
//
// One goal per lane, fp64 VALU, everything in registers, the joint loops fully
// unrolled: chain_solve_kernel<NJ, kLimited> is ik_refine.hip's kernel with NJ where
// that says 4 (the row functions are ik_chain_row.h, compiled by host programs too;
// kinematics/chain.py restates them), so at NJ = 4 without restarts it gives
// ik_refine's bits.  The table's constants and the limits come in one by-value struct
// and stay in scalar registers.
//
// Restarts are per lane: a lane whose attempt ends above tol with attempts left takes
// its next start point from the hash of (row, attempt, joint) and goes on; it keeps
// the best attempt's angles beside the current ones.  The wave iterates until no lane
// is active and there is no work queue, so converged lanes idle until their wave's
// slowest row ends -- the known cost of restarts.  HBM per row: 24 B goal +
// 8 NJ B seed in, 8 NJ B angles (+ 4 B steps + 4 B attempt + 8 B error) out; rows of
// odd NJ are not 16-byte aligned, so every access is 8 bytes.
#include "ik_chain.h"
#include "ik_fk_chain.h"
#include "ik_launch.h"
#include "ik_stats.h"

namespace ikhip {

constexpr double kChainClamp = 0.5;  // largest |delta_i| of one step, radians

template <int NJ, bool kLimited>
__global__ __launch_bounds__(256) void chain_solve_kernel(
    ChainParams P, ChainHome home, const double *pts, const double *seed, int64_t n, double tol,
    int max_iter, double lam2, int restarts, double *ang, int32_t *iters, int32_t *tries,
    double *fk_err, DevStats *S) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool valid = i < n;
  double px = 0.0, py = 0.0, pz = 0.0, t[NJ], best[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) t[j] = 0.0;
  if (valid) {
    px = pts[3 * i];
    py = pts[3 * i + 1];
    pz = pts[3 * i + 2];
#pragma unroll
    for (int j = 0; j < NJ; ++j)  // the seed (or the home pose), wrapped and projected
      t[j] = chain_place<kLimited>(seed ? seed[NJ * i + j] : home.th[j], P, j);
  }
#pragma unroll
  for (int j = 0; j < NJ; ++j) best[j] = t[j];
  const bool alpha_ok = !P.alpha_bad;  // some |alpha_i| > 2 pi: FK raises, the error is NaN

  bool active = valid;
  int it = 0, tot = 0;      // steps of this attempt, of all attempts
  int a = 0, best_try = 0;  // this attempt, the attempt `best` holds
  double err = 0.0, best_err = 0.0;
  for (;;) {
    double s[NJ], c[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) sincos_fk(t[j], &s[j], &c[j]);
    const ChainJacN<NJ> f = chain_jac<NJ>(P.jc, s, c);  // the effector and dFK / dtheta

    const double ex = px - f.x, ey = py - f.y, ez = pz - f.z;
    const double en = sqrt(ex * ex + ey * ey + ez * ez);
    bool fresh = false;  // t is a new start point: f is not its chain, no step this round
    if (active) {
      err = alpha_ok ? en : __builtin_nan("");
      if (!(err > tol) || it == max_iter) {  // the attempt ends
        if (a == 0 || err < best_err) {      // the smallest error, the earliest on a tie
          best_err = err;
          best_try = a;
#pragma unroll
          for (int j = 0; j < NJ; ++j) best[j] = t[j];
        }
        if (err > tol && a < restarts) {  // (a NaN error does not restart)
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

    // delta = J'^T (J' J'^T + lambda^2 I)^-1 e (ik_chain_row.h): every column, or
    // under joint limits without those the active-set loop locks
    double d[NJ];
    if constexpr (kLimited) {
      chain_step<NJ>(f, ex, ey, ez, lam2, t, P, d, nullptr);
    } else {
      chain_solve<NJ>(f, ex, ey, ez, lam2, 0u, d);
    }
    chain_scale<NJ>(d, kChainClamp);
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
    if (fk_err) fk_err[i] = best_err;
  }
  // n_capped: rows that did not converge (a NaN error included); first_err: the lowest
  // of them with a finite error
  const bool capped = valid && !(best_err <= tol);
  const bool finite = valid && best_err <= 1.7976931348623157e308;  // (not NaN)
  if (capped && finite) record_error(S, i, IK_E_OUT_OF_REACH);
  block_iter_stats_acc(S, valid ? (unsigned long long)tot : 0ull, capped ? 1ull : 0ull,
                       valid ? tot : 0);
  const double fe = finite ? best_err : 0.0;
  wave_fk_stats(S, fe, fe);
}

template <int NJ>
static void launch_chain_nj(const ChainParams &P, const ChainHome &home, const double *pts,
                            const double *seed, int64_t n, double tol, int max_iter,
                            double damping, int restarts, double *ang, int32_t *iters,
                            int32_t *tries, double *fk_err, DevStats *S, hipStream_t st) {
  const unsigned grid = (unsigned)((n + 255) / 256);
  // every joint free: the kernel without the limits' code
  if (P.mask) {
    kt_begin("chain_solve_limited_kernel", st);
    IK_LAUNCH((chain_solve_kernel<NJ, true>), dim3(grid), dim3(256), 0, st, P, home, pts, seed, n,
              tol, max_iter, damping * damping, restarts, ang, iters, tries, fk_err, S);
  } else {
    kt_begin("chain_solve_kernel", st);
    IK_LAUNCH((chain_solve_kernel<NJ, false>), dim3(grid), dim3(256), 0, st, P, home, pts, seed, n,
              tol, max_iter, damping * damping, restarts, ang, iters, tries, fk_err, S);
  }
  kt_end(st);
}

void launch_chain_solve(int nj, const ChainParams &P, const ChainHome &home, const double *pts,
                        const double *seed, int64_t n, double tol, int max_iter, double damping,
                        int restarts, double *ang, int32_t *iters, int32_t *tries,
                        double *fk_err, DevStats *S, hipStream_t st) {
  if (n <= 0) return;
#define IK_CHAIN_CASE(NJ)                                                                        \
  case NJ:                                                                                       \
    launch_chain_nj<NJ>(P, home, pts, seed, n, tol, max_iter, damping, restarts, ang, iters,     \
                        tries, fk_err, S, st);                                                   \
    break;
  switch (nj) {
    IK_CHAIN_CASE(2)
    IK_CHAIN_CASE(3)
    IK_CHAIN_CASE(4)
    IK_CHAIN_CASE(5)
    IK_CHAIN_CASE(6)
    IK_CHAIN_CASE(7)
    IK_CHAIN_CASE(8)
    default:
      break;  // (ik_chain_solve refuses other lengths)
  }
#undef IK_CHAIN_CASE
}

}  // namespace ikhip
