// ik_fabrik_plan.cpp -- see ik_fabrik_plan.h.  Host only (HOSTCXX).
#include "ik_fabrik_plan.h"

#include <cmath>

namespace ikhip {

// div_core's domain for the link lengths (the numerators): 2^-100 <= |L| <= 2^100.
bool links_core_ok(const double *L, int n) {
  for (int k = 0; k < n; ++k) {
    const double v = std::fabs(L[k]);
    if (!(v >= 0x1p-100 && v <= 0x1p100)) return false;
  }
  return true;
}

// The largest x with fl(sqrt(x)) <= tol (NaN for a NaN tol, -inf for a
// negative one), so that the reference's `sqrt(x) > tol` is `x > t` bit for
// bit.  The loop's initial errors of 1.0 stay 1.0 (sqrt(1) = 1 exactly).
double tol_threshold(double tol) {
  if (std::isnan(tol)) return NAN;
  if (tol < 0) return -INFINITY;
  if (std::isinf(tol)) return INFINITY;
  double t = tol * tol;
  while (std::sqrt(t) > tol) t = std::nextafter(t, -INFINITY);
  for (;;) {
    const double u = std::nextafter(t, INFINITY);
    if (std::sqrt(u) <= tol) t = u;
    else break;
  }
  return t;
}

// The band [lo, hi] of one launch (ik_fabrik_step.h, "the loop condition without
// the start and goal errors' own arithmetic", derives D and the two bounds).
ErrBand fabrik_band(double tol2, double n1max, double sum_l) {
  // tol2 <= 0 (tol = 0, or a negative tol): a band that decides nothing, every
  // comparison exact.  (hi = 0 would call any sea > 0 "above", but at tol = 0 the
  // reference stops where b0 rounds onto start exactly, se2 == 0, while s is
  // L0 +- 1 ulp and sea > 0: ADVICE r05.)
  ErrBand b = {-1.0, INFINITY};
  if (!(tol2 > 0.0)) return b;
  const double T = std::sqrt(tol2);
  const double tol_lo = T * (1.0 - 0x1p-50), tol_hi = T * (1.0 + 0x1p-50);
  const double d = 0x1p-52 * (6.0 * n1max + 8.0 * sum_l + 1.0);
  b.hi = (d + tol_hi) * (1.0 + 0x1p-36);
  b.lo = (d <= 0.5 * tol_lo) ? (tol_lo - d) * (1.0 - 0x1p-36) : -1.0;
  return b;
}

// qmax = min |L| 2^382 (ik_fabrik_step.h, "the core domain from the quotients").
double fabrik_qmax(const double *L) {
  double m = std::fabs(L[0]);
  for (int k = 1; k < 4; ++k) m = std::fmin(m, std::fabs(L[k]));
  return m * 0x1p382;
}

FabPlan fabrik_plan(const FabPlanIn &in) {
  constexpr double kPi = 3.141592653589793;  // math.pi (ik_types.h)
  const int64_t n = in.n;
  FabPlan p;
  p.tol2 = tol_threshold(in.tol);
  // the band covers goals well past the reach: 64 (1 + |d1| + |a1| + sum L)
  {
    const double sum_l = std::fabs(in.links[0]) + std::fabs(in.links[1]) +
                         std::fabs(in.links[2]) + std::fabs(in.links[3]);
    p.band_n1 = 64.0 * (1.0 + std::fabs(in.dh[4]) + std::fabs(in.dh[8]) + sum_l);
    if (!std::isfinite(p.band_n1)) p.band_n1 = -1.0;  // (no lane: every comparison exact)
    p.band = fabrik_band(p.tol2, p.band_n1, sum_l);
    p.qmax = fabrik_qmax(in.links);
  }
  // the seed's own angles (robot_const_kernel's check, forward.py:23-25)
  bool robot_ok = true;
  for (int k = 1; k < 4; ++k)
    if (in.dh[k] < -2 * kPi || in.dh[k] > 2 * kPi) robot_ok = false;
  for (int k = 0; k < 4; ++k)
    if (in.dh[12 + k] < -2 * kPi || in.dh[12 + k] > 2 * kPi) robot_ok = false;
  p.grid = (unsigned)((n + 255) / 256);
  // no iteration at all when the loop's initial errors of 1.0 already pass
  p.simple = in.variant == 0 || in.max_iter <= 0 || !(1.0 > p.tol2) || !robot_ok;
  if (p.simple) return p;
  p.ordered = in.has_table && in.order_env && n < (int64_t)1 << 31;
  if (p.ordered) p.ogrid = (unsigned)((n + 256 * in.ord_ppt - 1) / (256 * in.ord_ppt));
  // persistent grid: blocks_per_cu 256-thread blocks per CU (= waves per SIMD)
  // measured on MI355X (tools/sweep_fabrik.py): at 1M points 2 blocks/CU with
  // 64-point grabs beats 4 and 8 by 10-30 % (more lanes = fewer points per lane
  // = a longer divergent tail); 2 and 3 are within noise at 1-1.25M points, and
  // from 4M points on 3 wins by ~5 % at every tolerance (the tail matters less
  // than the latency a third wave per SIMD hides), and so it does at 1M points
  // with tol 1e-5 (56 iterations per point against 33 at 1e-3).
  // (4M / 10M points at tol 1e-3: 4 per CU is 2 % ahead of 3; at 1e-5 they are even)
  // bpc_req: the context's IKHIP_FABRIK_BPC (0 = this rule)
  // The fused kernel keeps the batch of prepared points and the angles step's
  // temporaries beside the loop state: ~250 VGPRs, two waves per SIMD at most.
  const int bpc =
      in.bpc_req > 0 ? (in.bpc_req < in.iter_waves ? in.bpc_req : in.iter_waves) : in.iter_waves;
  p.chunk = (in.chunk_env > 0 && in.chunk_env <= 64) ? in.chunk_env : 64;
  p.pgrid = (unsigned)in.cus * (unsigned)(bpc > 0 ? bpc : 8);
  int64_t waves_needed = (n + 63) / 64;
  if ((int64_t)p.pgrid * 4 > waves_needed)
    p.pgrid = (unsigned)((waves_needed + 3) / 4 > 0 ? (waves_needed + 3) / 4 : 1);
  // the iteration through sqrt_core / div_core (same bits, fewer instructions)
  // unless the link lengths are outside div_core's domain, and with the repeated
  // distances taken once (core 2) when L0 == L1 and L2 == L3.  core_req (context's
  // IKHIP_FABRIK_CORE) 0 forces the general sqrt / division, 1 the core sequences
  // without the reuse.
  const double *Lk = in.links;
  p.core = links_core_ok(Lk, 4) ? in.core_req : 0;
  if (p.core == 2 && !(Lk[0] == Lk[1] && Lk[2] == Lk[3])) p.core = 1;
  p.refill1 = in.variant == 2;
  return p;
}

}  // namespace ikhip
