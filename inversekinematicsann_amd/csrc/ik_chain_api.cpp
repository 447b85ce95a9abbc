// ik_chain_api.cpp -- ik_chain_solve and ik_chain_pose_solve of the C ABI (declared in
// include/ikhip.h; kernels: ik_chain.hip, ik_chain_pose.hip).  The call bodies only:
// the refused arguments, the table's constants and limits as the kernels take them (by
// value: no upload, so an IK_F_ASYNC call adds no copy and no sync), the staging of the
// arrays.  Neither reads nor changes the context's robot, its workspace limits or its
// stored joint limits.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "ik_chain.h"
#include "ik_chain_pose.h"
#include "ik_fk.h"
#include "ik_internal.h"

using namespace ikhip;
using namespace ikapi;

// What both calls refuse after refine_args, under the call's own name `w`, and the
// table's constants, limits and home pose as the kernels take them.
static int chain_params(const std::string &w, int nj, const double *dh, const double *lo,
                        const double *hi, int32_t max_iter, int32_t restarts, ChainParams &P,
                        ChainHome &home) {
  if (nj < kChainMinJoints || nj > kChainMaxJoints)
    return fail(IK_E_BADARG, w + "nj " + std::to_string(nj) + " is outside 2..8 (longer chains "
                                 "are not built)");
  if (!dh) return fail(IK_E_BADARG, w + "dh is NULL");
  if (restarts < 0 || restarts > 255)
    return fail(IK_E_BADARG, w + "restarts " + std::to_string(restarts) + " is outside 0..255");
  // a row counts the steps of all its attempts in an int32 (iters, max_iters)
  if ((int64_t)max_iter * (restarts + 1) > INT32_MAX)
    return fail(IK_E_BADARG, w + "max_iter * (restarts + 1) exceeds 2^31 - 1, the steps a row "
                                 "can count");
  if (!lo != !hi)
    return fail(IK_E_BADARG, w + "lo and hi must both be given or both be NULL");
  P = {};
  home = {};
  for (int i = 0; i < kChainMaxJoints; ++i) {
    P.lo[i] = -HUGE_VAL;
    P.hi[i] = HUGE_VAL;
  }
  for (int i = 0; i < nj; ++i) {
    const double d = dh[nj + i], a = dh[2 * nj + i], al = dh[3 * nj + i];
    if (!std::isfinite(d) || !std::isfinite(a) || !std::isfinite(al))
      return fail(IK_E_BADARG, w + "joint " + std::to_string(i + 1) +
                                   ": a non-finite entry in the d, a or alpha rows of dh");
    // fk_trip_consts' values: {a, d, cos alpha, sin alpha} in float64 on the host
    P.jc[i][0] = a;
    P.jc[i][1] = d;
    P.jc[i][2] = std::cos(al);
    P.jc[i][3] = std::sin(al);
    if (al < -2 * kPi || al > 2 * kPi) P.alpha_bad = 1;
    home.th[i] = dh[i];
  }
  for (int i = 0; lo && i < nj; ++i) {  // ik_set_joint_limits' rule, per joint
    const std::string who = w + "joint " + std::to_string(i + 1) + ": ";
    if (std::isnan(lo[i]) || std::isnan(hi[i])) return fail(IK_E_BADARG, who + "a bound is NaN");
    if (lo[i] == -HUGE_VAL && hi[i] == HUGE_VAL) continue;  // free
    if (std::isinf(lo[i]) != std::isinf(hi[i]))
      return fail(IK_E_BADARG, who + "one bound is infinite and the other finite");
    if (lo[i] > hi[i]) return fail(IK_E_BADARG, who + "lo > hi");
    if (lo[i] < -kPi || hi[i] > kPi)
      return fail(IK_E_BADARG, who + "a bound lies outside [-pi, pi]");
    P.lo[i] = lo[i];
    P.hi[i] = hi[i];
    P.mask |= 1u << i;
  }
  return IK_OK;
}

extern "C" int ik_chain_solve(ik_ctx *c, int nj, const double *dh, const double *lo,
                              const double *hi, const double *pts, const double *seed, int64_t n,
                              double tol, int32_t max_iter, double damping, int32_t restarts,
                              double *ang, int32_t *iters, int32_t *tries, double *fk_err,
                              int flags, ik_stats *stats) {
  // (no alignment is demanded of ang: rows of odd nj have none, the kernel stores 8 bytes)
  int rc = refine_args("ik_chain_solve", c, n, pts && ang, tol, max_iter, damping, nullptr, flags);
  if (rc) return rc;
  ChainParams P;
  ChainHome home;
  if ((rc = chain_params("ik_chain_solve: ", nj, dh, lo, hi, max_iter, restarts, P, home)))
    return rc;
  if ((rc = set_dev(c))) return rc;
  KtScope kts(c);
  Stage st(c, flags);
  const size_t row = (size_t)nj * sizeof(double);
  const int r_pts = st.in(pts, (size_t)n * 24);
  const int r_seed = seed ? st.in(seed, (size_t)n * row) : -1;
  const int r_ang = st.out(ang, (size_t)n * row), r_it = st.out(iters, (size_t)n * 4),
            r_tr = st.out(tries, (size_t)n * 4), r_fe = st.out(fk_err, (size_t)n * 8);
  if ((rc = st.reserve())) return rc;
  launch_reset_stats(c->d_stats, c->stream);
  launch_chain_solve(nj, P, home, st.at<const double>(r_pts),
                     r_seed >= 0 ? st.at<const double>(r_seed) : nullptr, n, tol, max_iter,
                     damping, restarts, st.at<double>(r_ang), st.at<int32_t>(r_it),
                     st.at<int32_t>(r_tr), st.at<double>(r_fe), c->d_stats, c->stream);
  IK_HIP(hipGetLastError());
  if ((rc = st.flush())) return rc;
  return finish(c, flags, stats);
}

extern "C" int ik_chain_pose_solve(ik_ctx *c, int nj, const double *dh, const double *lo,
                                   const double *hi, const double *pts, const double *rot,
                                   const double *seed, int64_t n, double tol, double rot_tol,
                                   double rot_weight, int32_t max_iter, double damping,
                                   int32_t restarts, double *ang, int32_t *iters, int32_t *tries,
                                   double *fk_err, double *rot_err, int flags, ik_stats *stats) {
  const std::string w = "ik_chain_pose_solve: ";
  int rc = refine_args("ik_chain_pose_solve", c, n, pts && ang, tol, max_iter, damping, nullptr,
                       flags);
  if (rc) return rc;
  if (n > 0 && !rot) return fail(IK_E_BADARG, w + "rot is NULL");
  if (std::isnan(rot_tol)) return fail(IK_E_BADARG, w + "rot_tol is NaN");
  if (!std::isfinite(rot_weight) || rot_weight < 0.0)
    return fail(IK_E_BADARG, w + "rot_weight must be finite and >= 0");
  ChainParams P;
  ChainHome home;
  if ((rc = chain_params(w, nj, dh, lo, hi, max_iter, restarts, P, home))) return rc;
  if ((rc = set_dev(c))) return rc;
  KtScope kts(c);
  Stage st(c, flags);
  const size_t row = (size_t)nj * sizeof(double);
  const int r_pts = st.in(pts, (size_t)n * 24), r_rot = st.in(rot, (size_t)n * 72);
  const int r_seed = seed ? st.in(seed, (size_t)n * row) : -1;
  const int r_ang = st.out(ang, (size_t)n * row), r_it = st.out(iters, (size_t)n * 4),
            r_tr = st.out(tries, (size_t)n * 4), r_fe = st.out(fk_err, (size_t)n * 8),
            r_re = st.out(rot_err, (size_t)n * 8);
  if ((rc = st.reserve())) return rc;
  launch_reset_stats(c->d_stats, c->stream);
  launch_chain_pose_solve(nj, P, home, st.at<const double>(r_pts), st.at<const double>(r_rot),
                          r_seed >= 0 ? st.at<const double>(r_seed) : nullptr, n, tol, rot_tol,
                          rot_weight, max_iter, damping, restarts, st.at<double>(r_ang),
                          st.at<int32_t>(r_it), st.at<int32_t>(r_tr), st.at<double>(r_fe),
                          st.at<double>(r_re), c->d_stats, c->stream);
  IK_HIP(hipGetLastError());
  if ((rc = st.flush())) return rc;
  return finish(c, flags, stats);
}
