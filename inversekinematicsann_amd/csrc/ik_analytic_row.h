// ik_analytic_row.h -- one row of ik_analytic_solve: the closed-form inverse of a
// yaw joint followed by a planar three-link chain, for a goal, a tool pitch
// phi = theta2 + theta3 + theta4 and an elbow branch b = -1 / +1 (include/ikhip.h
// "Analytic" states the arithmetic; kinematics/analytic.py restates it in numpy).
// Compiled by the kernel (ik_analytic.hip) and by a plain host compiler
// (tests/host/analytic_check.cpp): sqrt / atan2 / acos / sin / cos are libm there
// and the device library here, everything else is the same IEEE operation in the
// same order (-ffp-contract=off).
//
// m = 1 - cos(theta3) and q = 1 + cos(theta3) are kept as products of the sums and
// differences of the lengths: a folded (q -> 0) or stretched (m -> 0) elbow then
// loses nothing to cancellation, where c3 = (W^2 - a2^2 - a3^2) / (2 a2 a3) with
// s3 = sqrt(1 - c3^2) loses about eps a2 a3 / W.
#pragma once

#include "ik_analytic_plan.h"
#include "ik_row.h"

namespace ikhip {

struct AnalyticRow {
  double t1, t2, t3, t4;  // NaN when the row failed
  double phi;             // the pitch used (NaN when the row failed)
  bool fail, moved;
};

struct AnalyticWrist {
  double wr, wh, m, q;
};

IK_ROW_FN AnalyticWrist analytic_wrist(const AnalyticRobot &R, double r, double h, double phi) {
  const double sa = R.a2 + R.a3, da = fabs(R.a2 - R.a3), k2 = 2 * R.a2 * R.a3;
  AnalyticWrist w;
  w.wr = r - R.a4 * cos(phi);
  w.wh = h - R.a4 * sin(phi);
  const double W = sqrt(w.wr * w.wr + w.wh * w.wh);
  w.m = (sa - W) * (sa + W) / k2;
  w.q = (W - da) * (W + da) / k2;
  return w;
}

// has_pitch false: phi = gamma, the tool points away from the shoulder.
IK_ROW_FN AnalyticRow analytic_row(const AnalyticRobot &R, double x, double y, double z,
                                   bool has_pitch, double pitch, double b, bool nearest) {
  AnalyticRow o;
  o.t1 = atan2(y, x);
  const double r = sqrt(x * x + y * y) - R.a1, h = z - R.d1;
  const double rho2 = r * r + h * h, rho = sqrt(rho2), gam = atan2(h, r);
  double phi = has_pitch ? pitch : gam;
  AnalyticWrist w = analytic_wrist(R, r, h, phi);
  const bool infeasible = !(w.m >= 0.0 && w.q >= 0.0);  // (a NaN row is infeasible)
  o.fail = infeasible;
  o.moved = false;
  if (nearest && infeasible) {
    // |phi - gamma| must lie in [lo, hi] for the wrist to fall between the rings
    // |a2 - a3| <= W <= a2 + a3: move phi to the nearer end on its own side
    const double sa = R.a2 + R.a3, da = fabs(R.a2 - R.a3), den = 2 * R.a4 * rho;
    const double cmin = (rho2 + R.a4 * R.a4 - sa * sa) / den;
    const double cmax = (rho2 + R.a4 * R.a4 - da * da) / den;
    const double dl = wrap_pi(phi - gam);
    // (dl == dl: a NaN or infinite pitch has no nearest one)
    const bool any = cmin <= 1.0 && cmax >= -1.0 && rho > 0.0 && dl == dl;
    if (any) {
      const double lo = acos(cmax < 1.0 ? cmax : 1.0), hi = acos(cmin > -1.0 ? cmin : -1.0);
      double ad = fabs(dl);
      ad = ad < lo ? lo : ad;
      ad = ad > hi ? hi : ad;
      phi = gam + (dl < 0.0 ? -1.0 : 1.0) * ad;
      w = analytic_wrist(R, r, h, phi);
      w.m = w.m > 0.0 ? w.m : 0.0;
      w.q = w.q > 0.0 ? w.q : 0.0;
      o.fail = false;
      o.moved = true;
    }
  }
  const double s3 = b * sqrt(w.m * w.q), c3 = (w.q - w.m) / 2;
  o.t3 = b * 2 * atan2(sqrt(w.m), sqrt(w.q));
  const double t2 = atan2(w.wh, w.wr) - atan2(R.a3 * s3, R.a2 + R.a3 * c3);
  o.t4 = wrap_pi(phi - t2 - o.t3);
  o.t2 = wrap_pi(t2);
  o.phi = phi;
  if (o.fail) o.t1 = o.t2 = o.t3 = o.t4 = o.phi = __builtin_nan("");
  return o;
}

}  // namespace ikhip
