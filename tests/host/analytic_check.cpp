// analytic_check.cpp -- the host side of ik_analytic_solve on the CPU: the
// acceptance rule of csrc/ik_analytic_plan.cpp on a table of DH matrices, and the
// row function of csrc/ik_analytic_row.h (the one the kernel compiles) on rows the
// Python test passes in.  Stand-alone, built with AddressSanitizer +
// UndefinedBehaviorSanitizer by tests/test_analytic_cpu.py and run directly.
//
//   analytic_check                 the acceptance table, then "analytic_check ok"
//   analytic_check ROWS            also solves every line of the file ROWS,
//       d1 a1 a2 a3 a4 x y z has_pitch pitch elbow nearest
//     and prints one line per row, "row t1 t2 t3 t4 phi fail moved" (%.17g), before
//     the ok line; the test compares them with the numpy restatement.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "ik_analytic_plan.h"
#include "ik_analytic_row.h"

using namespace ikhip;

static int g_bad = 0;
#define CHECK(cond, ...)                        \
  do {                                          \
    if (!(cond)) {                              \
      std::printf("FAILED %s: ", #cond);        \
      std::printf(__VA_ARGS__);                 \
      std::printf("\n");                        \
      ++g_bad;                                  \
    }                                           \
  } while (0)

static const double kHalfPi = 3.141592653589793 / 2;

struct Table {
  double dh[16];
};

static Table sixdof() {
  return {{0.0, kHalfPi, 0.0, 0.0, 2.0, 0.0, 0.0, 0.0, 0.0, 2.0, 2.0, 2.0, kHalfPi, 0.0, 0.0, 0.0}};
}
static Table planar2() {
  return {{0.0, kHalfPi, 0.0, 0.0, 0.7, 0.0, 0.0, 0.0, 0.3, 1.5, 2.5, 1.0, kHalfPi, 0.0, 0.0, 0.0}};
}
static Table skew() {
  return {{0.0, kHalfPi, 0.0, 0.0, 2.0, 0.0, 0.3, 0.0, 0.0, 2.0, 2.0, 2.0, kHalfPi, 0.4, 0.0, 0.0}};
}

// One entry of the six-DOF table replaced: refused, and the message names `name`.
static void refused(int at, double v, const char *name) {
  Table t = sixdof();
  t.dh[at] = v;
  AnalyticRobot r = {-1, -1, -1, -1, -1};
  const std::string why = analytic_robot(t.dh, &r);
  CHECK(!why.empty(), "dh[%d] = %g accepted", at, v);
  CHECK(why.rfind(name, 0) == 0, "dh[%d] = %g: message '%s' does not start with %s", at, v,
        why.c_str(), name);
  CHECK(r.d1 == -1 && r.a4 == -1, "dh[%d] = %g: *out written on refusal", at, v);
}

static void accepted(const Table &t, const AnalyticRobot &want, const char *what) {
  AnalyticRobot r = {};
  const std::string why = analytic_robot(t.dh, &r);
  CHECK(why.empty(), "%s refused: %s", what, why.c_str());
  CHECK(r.d1 == want.d1 && r.a1 == want.a1 && r.a2 == want.a2 && r.a3 == want.a3 &&
            r.a4 == want.a4,
        "%s: lengths %g %g %g %g %g", what, r.d1, r.a1, r.a2, r.a3, r.a4);
}

static void acceptance() {
  accepted(sixdof(), {2.0, 0.0, 2.0, 2.0, 2.0}, "SixDOFRobot");
  accepted(planar2(), {0.7, 0.3, 1.5, 2.5, 1.0}, "PLANAR2");
  {
    Table t = skew();
    AnalyticRobot r;
    const std::string why = analytic_robot(t.dh, &r);
    CHECK(why.rfind("alpha2", 0) == 0, "SKEW_DH: '%s'", why.c_str());
  }
  // the theta row is not read; -0 is 0
  {
    Table t = sixdof();
    t.dh[0] = 1.25, t.dh[1] = NAN, t.dh[13] = -0.0, t.dh[6] = -0.0;
    accepted(t, {2.0, 0.0, 2.0, 2.0, 2.0}, "theta row / -0");
  }
  const double inf = INFINITY;
  // each single violation (rows theta, d, a, alpha: d at 4.., a at 8.., alpha at 12..)
  refused(12, -kHalfPi, "alpha1");  // sin alpha1 < 0
  refused(12, kHalfPi + 1e-9, "alpha1");  // |cos alpha1| = 1e-9
  refused(12, 0.0, "alpha1");
  refused(12, NAN, "alpha1");
  refused(13, 0.4, "alpha2");
  refused(14, -1e-300, "alpha3");
  refused(15, NAN, "alpha4");
  refused(5, 0.3, "d2");
  refused(6, -0.3, "d3");
  refused(7, NAN, "d4");
  refused(9, 0.0, "a2");
  refused(9, NAN, "a2");
  refused(10, -2.0, "a3");
  refused(10, inf, "a3");
  refused(11, 0.0, "a4");
  refused(8, -1e-9, "a1");
  refused(8, inf, "a1");
  refused(8, NAN, "a1");
}

// Rows whose result is exact whatever libm's last bits are.
static void exact_rows() {
  const AnalyticRobot R = {2.0, 0.0, 2.0, 2.0, 2.0};
  for (double b : {-1.0, 1.0}) {
    // full stretch: m = 0, every angle 0
    AnalyticRow o = analytic_row(R, 6.0, 0.0, 2.0, false, 0.0, b, false);
    CHECK(!o.fail && !o.moved && o.t1 == 0 && o.t2 == 0 && o.t3 == 0 && o.t4 == 0 && o.phi == 0,
          "full stretch b %g: %g %g %g %g", b, o.t1, o.t2, o.t3, o.t4);
    // folded onto the shoulder's link: W = 0, theta3 = b pi, theta4 = -b pi
    o = analytic_row(R, 2.0, 0.0, 2.0, false, 0.0, b, false);
    CHECK(!o.fail && o.t1 == 0 && o.t2 == 0 && o.t3 == b * 3.141592653589793 &&
              o.t4 == -b * 3.141592653589793,
          "folded b %g: %g %g %g %g", b, o.t1, o.t2, o.t3, o.t4);
    // beyond reach fails in both modes, a NaN goal and a NaN / infinite pitch too
    for (bool nearest : {false, true}) {
      o = analytic_row(R, 7.0, 0.0, 2.0, false, 0.0, b, nearest);
      CHECK(o.fail && !o.moved && std::isnan(o.t1) && std::isnan(o.t4) && std::isnan(o.phi),
            "beyond reach, nearest %d", (int)nearest);
      o = analytic_row(R, NAN, 1.0, 1.0, false, 0.0, b, nearest);
      CHECK(o.fail && !o.moved && std::isnan(o.t3), "NaN goal, nearest %d", (int)nearest);
      for (double ph : {(double)NAN, (double)INFINITY}) {
        o = analytic_row(R, 4.0, 0.0, 2.0, true, ph, b, nearest);
        CHECK(o.fail && !o.moved && std::isnan(o.t2) && std::isnan(o.phi),
              "pitch %g, nearest %d", ph, (int)nearest);
      }
    }
    // a pitch that points the tool back at the shoulder: infeasible, moved when asked
    o = analytic_row(R, 5.5, 0.0, 2.0, true, 3.0, b, false);
    CHECK(o.fail && !o.moved, "strict infeasible pitch");
    o = analytic_row(R, 5.5, 0.0, 2.0, true, 3.0, b, true);
    // (the moved pitch stretches the arm: m is 0 up to rounding, theta3 ~ sqrt(2 m))
    CHECK(!o.fail && o.moved && o.phi > 0.59 && o.phi < 0.60 && std::fabs(o.t3) < 1e-6,
          "nearest pitch: phi %g t3 %g", o.phi, o.t3);
  }
}

static int solve_file(const char *path) {
  std::FILE *f = std::fopen(path, "r");
  if (!f) {
    std::printf("cannot open %s\n", path);
    return 1;
  }
  char line[1024];
  int rows = 0;
  while (std::fgets(line, sizeof(line), f)) {
    double v[12];
    int got = 0;
    char *p = line;
    for (; got < 12; ++got) {
      char *end;
      v[got] = std::strtod(p, &end);
      if (end == p) break;
      p = end;
    }
    if (got == 0) continue;
    if (got != 12) {
      std::printf("row %d: %d of 12 fields\n", rows, got);
      std::fclose(f);
      return 1;
    }
    const AnalyticRobot R = {v[0], v[1], v[2], v[3], v[4]};
    const AnalyticRow o = analytic_row(R, v[5], v[6], v[7], v[8] != 0.0, v[9], v[10], v[11] != 0.0);
    std::printf("row %.17g %.17g %.17g %.17g %.17g %d %d\n", o.t1, o.t2, o.t3, o.t4, o.phi,
                (int)o.fail, (int)o.moved);
    ++rows;
  }
  std::fclose(f);
  std::printf("rows %d\n", rows);
  return 0;
}

int main(int argc, char **argv) {
  acceptance();
  exact_rows();
  if (argc > 1 && solve_file(argv[1])) return 1;
  if (g_bad) {
    std::printf("analytic_check: %d checks failed\n", g_bad);
    return 1;
  }
  std::printf("analytic_check ok\n");
  return 0;
}
