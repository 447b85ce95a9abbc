// ik_analytic_plan.cpp -- see ik_analytic_plan.h.
#include "ik_analytic_plan.h"

#include <cmath>
#include <cstdio>

namespace ikhip {

static std::string entry(const char *name, int joint, double v, const char *rule) {
  char buf[160];
  std::snprintf(buf, sizeof(buf), "%s%d = %.17g %s", name, joint, v, rule);
  return buf;
}

std::string analytic_robot(const double dh[16], AnalyticRobot *out) {
  const double *d = dh + 4, *a = dh + 8, *al = dh + 12;
  // (negated comparisons: a NaN entry is refused)
  if (!(std::fabs(std::cos(al[0])) <= 1e-12) || !(std::sin(al[0]) > 0.0))
    return entry("alpha", 1, al[0], "must be +pi/2 (|cos| <= 1e-12, sin > 0)");
  for (int i = 1; i < 4; ++i)
    if (!(al[i] == 0.0)) return entry("alpha", i + 1, al[i], "must be 0");
  for (int i = 1; i < 4; ++i)
    if (!(d[i] == 0.0)) return entry("d", i + 1, d[i], "must be 0");
  for (int i = 1; i < 4; ++i)
    if (!std::isfinite(a[i]) || !(a[i] > 0.0)) return entry("a", i + 1, a[i], "must be finite and > 0");
  if (!std::isfinite(a[0]) || !(a[0] >= 0.0)) return entry("a", 1, a[0], "must be finite and >= 0");
  *out = {d[0], a[0], a[1], a[2], a[3]};
  return "";
}

}  // namespace ikhip
