// ik_analytic_plan.h -- the host side of ik_analytic_solve (ik_analytic.hip): which
// DH tables are "a yaw joint followed by a planar three-link chain", and the five
// lengths the closed form needs.  Plain C++, no HIP header, no state: tested on the
// CPU (tests/test_analytic_cpu.py, tests/host/analytic_check.cpp).
#pragma once

#include <string>

namespace ikhip {

// d1 = d[0], a1..a4 = a[0..3] of the DH table (rows theta, d, a, alpha).
struct AnalyticRobot {
  double d1, a1, a2, a3, a4;
};

// Accepted when |cos alpha1| <= 1e-12 and sin alpha1 > 0, alpha2 = alpha3 = alpha4 = 0,
// d2 = d3 = d4 = 0, a2 / a3 / a4 finite and > 0, a1 finite and >= 0 (the theta row
// is not read).  Returns "" and fills *out, or a message naming the first entry
// that breaks the rule (*out is then untouched).
std::string analytic_robot(const double dh[16], AnalyticRobot *out);

}  // namespace ikhip
