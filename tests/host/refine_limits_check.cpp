// refine_limits_check.cpp -- the step of the limited refine on the CPU: the row
// functions of csrc/ik_refine_step.h (the ones the kernel compiles) on a few rows
// whose outcome is known, and on rows the Python test passes in.  Stand-alone, built
// with AddressSanitizer + UndefinedBehaviorSanitizer by
// tests/test_refine_limits_cpu.py and run directly.
//
//   refine_limits_check            the built-in rows, then "refine_limits_check ok"
//   refine_limits_check ROWS       also runs refine_step on every line of the file ROWS,
//       j0x j0y j1x j1y j1z j2x j2y j2z j3x j3y j3z  ex ey ez  t0..t3  lo0..lo3  hi0..hi3
//       mask lam2                  (C99 hexadecimal floats, inf for a free joint's bounds)
//     and prints one line per row, "row d0 d1 d2 d3 lock resolves" (%a), before the
//     ok line; the test compares them bit for bit with the numpy restatement.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "ik_refine_step.h"

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

static const double kPiD = 3.141592653589793;
static const double kInf = INFINITY;

static bool same_bits(const double *a, const double *b, int n) {
  return std::memcmp(a, b, (size_t)n * sizeof(double)) == 0;
}

static void builtin_rows() {
  // a well-conditioned Jacobian (the stretched-up arm turned a little)
  const RefineJ J = {-0.3, 1.9, 0.7, 0.1, -1.2, 0.5, 0.08, -0.9, 0.2, 0.03, -0.4};
  const double ex = 0.01, ey = -0.02, ez = 0.015, lam2 = 1e-6;
  double free_d[4], d[4];
  refine_solve(J, ex, ey, ez, lam2, 0u, free_d);
  for (int i = 0; i < 4; ++i) CHECK(std::isfinite(free_d[i]), "free delta %d = %g", i, free_d[i]);

  // limits that do not bind: no lock, no re-solve, the free solve's bits
  {
    const JointLimits L = {{-kPiD, -kPiD, -kPiD, -kPiD}, {kPiD, kPiD, kPiD, kPiD}, 15u};
    const double t[4] = {0.1, 0.2, -0.3, 0.4};
    int rs = -1;
    const unsigned lock = refine_step(J, ex, ey, ez, lam2, t, L, d, &rs);
    CHECK(lock == 0 && rs == 0 && same_bits(d, free_d, 4), "never-binding: lock %u resolves %d",
          lock, rs);
  }
  // every joint free: bounds at infinity never lock, wherever theta is
  {
    const JointLimits L = {{-kInf, -kInf, -kInf, -kInf}, {kInf, kInf, kInf, kInf}, 0u};
    const double t[4] = {kPiD, -kPiD, 0.0, 0.0};
    int rs = -1;
    const unsigned lock = refine_step(J, ex, ey, ez, lam2, t, L, d, &rs);
    CHECK(lock == 0 && rs == 0 && same_bits(d, free_d, 4), "all free: lock %u", lock);
  }
  // a fixed joint 4 with a non-zero delta locks at once; its delta becomes a zero and
  // the others solve the 3-column system
  {
    JointLimits L = {{-kInf, -kInf, -kInf, 0.25}, {kInf, kInf, kInf, 0.25}, 8u};
    const double t[4] = {0.1, 0.2, -0.3, 0.25};
    int rs = -1;
    const unsigned lock = refine_step(J, ex, ey, ez, lam2, t, L, d, &rs);
    CHECK(free_d[3] != 0.0, "the free delta of joint 4 is zero");
    CHECK(lock == 8u && rs == 1 && d[3] == 0.0, "fixed joint: lock %u resolves %d d3 %g", lock, rs,
          d[3]);
    double want[4];
    refine_solve(J, ex, ey, ez, lam2, 8u, want);
    CHECK(same_bits(d, want, 4), "fixed joint: not the masked solve");
    // a joint on its bound whose delta points inwards stays free
    L.lo[3] = free_d[3] > 0.0 ? 0.25 : -1.0;
    L.hi[3] = free_d[3] > 0.0 ? 1.0 : 0.25;
    CHECK(refine_step(J, ex, ey, ez, lam2, t, L, d, &rs) == 0 && rs == 0 && same_bits(d, free_d, 4),
          "inward delta locked");
  }
  // every joint locked: A = lam2 I, delta all zero, finite
  {
    const JointLimits L = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}, 15u};
    const double t[4] = {0.0, 0.0, 0.0, 0.0};
    int rs = -1;
    const unsigned lock = refine_step(J, ex, ey, ez, lam2, t, L, d, &rs);
    CHECK(lock == 15u && rs >= 1 && rs <= 4, "all fixed: lock %u resolves %d", lock, rs);
    for (int i = 0; i < 4; ++i) CHECK(d[i] == 0.0, "all fixed: delta %d = %g", i, d[i]);
  }
  // the projection: inside untouched (the bits, -0.0 too), outside onto the bound, NaN kept
  CHECK(refine_project(0.3, -1.0, 1.0) == 0.3 && refine_project(-2.0, -1.0, 1.0) == -1.0 &&
            refine_project(2.0, -1.0, 1.0) == 1.0 && refine_project(5.0, 0.25, 0.25) == 0.25,
        "refine_project");
  CHECK(std::signbit(refine_project(-0.0, 0.0, 1.0)), "refine_project(-0.0)");
  CHECK(std::isnan(refine_project(NAN, -1.0, 1.0)), "refine_project(NaN)");
}

static int step_file(const char *path) {
  std::FILE *f = std::fopen(path, "r");
  if (!f) {
    std::printf("cannot open %s\n", path);
    return 1;
  }
  char line[2048];
  int rows = 0;
  while (std::fgets(line, sizeof(line), f)) {
    double v[28];
    int got = 0;
    char *p = line;
    for (; got < 28; ++got) {
      char *end;
      v[got] = std::strtod(p, &end);
      if (end == p) break;
      p = end;
    }
    if (got == 0) continue;
    if (got != 28) {
      std::printf("row %d: %d of 28 fields\n", rows, got);
      std::fclose(f);
      return 1;
    }
    const RefineJ J = {v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9], v[10]};
    const double t[4] = {v[14], v[15], v[16], v[17]};
    JointLimits L;
    for (int i = 0; i < 4; ++i) {
      L.lo[i] = v[18 + i];
      L.hi[i] = v[22 + i];
    }
    L.mask = (unsigned)v[26];
    double d[4];
    int rs = 0;
    const unsigned lock = refine_step(J, v[11], v[12], v[13], v[27], t, L, d, &rs);
    std::printf("row %a %a %a %a %u %d\n", d[0], d[1], d[2], d[3], lock, rs);
    ++rows;
  }
  std::fclose(f);
  std::printf("rows %d\n", rows);
  return 0;
}

int main(int argc, char **argv) {
  builtin_rows();
  if (argc > 1 && step_file(argv[1])) return 1;
  if (g_bad) {
    std::printf("refine_limits_check: %d checks failed\n", g_bad);
    return 1;
  }
  std::printf("refine_limits_check ok\n");
  return 0;
}
