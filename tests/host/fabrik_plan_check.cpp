// fabrik_plan_check.cpp -- CPU check of csrc/ik_fabrik_plan.cpp, built with
// -fsanitize=address,undefined by tests/test_fabrik_plan_cpu.py.
//
// tol_threshold is checked by its definition (the largest x with
// fl(sqrt(x)) <= tol) over every binade, fabrik_band by the properties the
// iteration relies on, fabrik_qmax exactly, and the plan against expectations
// written out case by case below, never by a copy of the plan's code.
// With --band the program prints fabrik_band's results for a fixed list of
// (tol2, n1max, sum_l) as hex floats, one "tol2 n1max sum_l lo hi" per line:
// tests/test_band_cpu.py holds its Python restatement to them bit for bit.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>

#include "ik_fabrik_plan.h"

using namespace ikhip;

static int g_fail = 0;
#define CHECK(cond, ...)                                 \
  do {                                                   \
    if (!(cond)) {                                       \
      if (++g_fail <= 20) {                              \
        std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
        std::printf(__VA_ARGS__);                        \
        std::printf("\n");                               \
      }                                                  \
    }                                                    \
  } while (0)

static const double kInf = INFINITY;

// ---- tol_threshold ---------------------------------------------------------
static long g_tols = 0;
static void check_tol(double tol) {  // tol >= 0 (or -0.0), finite
  const double t = tol_threshold(tol);
  ++g_tols;
  CHECK(std::sqrt(t) <= tol, "tol %a: sqrt(t = %a) > tol", tol, t);
  if (t != DBL_MAX)
    CHECK(std::sqrt(std::nextafter(t, kInf)) > tol, "tol %a: t = %a is not the largest", tol, t);
}

static void check_tol_threshold() {
  std::mt19937_64 rng(20240607);
  auto unit = [&]() { return (double)(rng() >> 11) * 0x1p-53; };  // [0, 1)
  for (int e = -1074; e <= 1023; ++e) {
    const double p2 = std::ldexp(1.0, e);
    check_tol(p2);
    check_tol(std::nextafter(p2, 0.0));
    for (int k = 0; k < 64; ++k) check_tol(std::ldexp(1.0 + unit(), e));
  }
  for (int k = 0; k < 2000000; ++k) check_tol(1e-7 + unit() * (1.0 - 1e-7));
  const double sp[] = {0.0, -0.0, 1e-3, 1e-5, 1.0, DBL_MAX, 0x1p-1074};
  for (double tol : sp) check_tol(tol);
  CHECK(g_tols > 2100000, "the sweep ran %ld values", g_tols);
  CHECK(std::isnan(tol_threshold(NAN)), "NaN tol");
  CHECK(tol_threshold(-1.0) == -kInf && tol_threshold(-0x1p-1074) == -kInf &&
            tol_threshold(-kInf) == -kInf,
        "negative tol");
  CHECK(tol_threshold(kInf) == kInf, "+inf tol");
  CHECK(tol_threshold(0.0) == 0.0 && tol_threshold(-0.0) == 0.0, "zero tol");
}

// ---- fabrik_band -----------------------------------------------------------
struct Triple {
  double tol2, n1max, sum_l;
};

// The --band list (and the property sweep's): the thresholds of common and tight
// tolerances, extreme ones, the specials, against the default launch's n1max
// (64 * 11), a small and a large robot's, and the "no lane" value -1.
static int band_list(Triple *out) {
  const double tol2s[] = {tol_threshold(1e-3), tol_threshold(1e-5), tol_threshold(1e-13),
                          tol_threshold(1e-7), tol_threshold(1e-9), tol_threshold(0.5),
                          1e-6, 0x1p-1074, DBL_MIN, 1e-300, 0x1.fffffffffffffp-1, DBL_MAX,
                          0.0, -0.0, -1.0, -kInf, NAN};
  const double nl[][2] = {{64.0 * 11.0, 8.0}, {-1.0, 8.0}, {64.0 * 1.004, 0.004}, {6.4e7, 3e5}};
  int m = 0;
  for (double t2 : tol2s)
    for (const double *p : nl) out[m++] = {t2, p[0], p[1]};
  return m;
}

static void check_band_props(const Triple &c) {
  const ErrBand b = fabrik_band(c.tol2, c.n1max, c.sum_l);
  if (!(c.tol2 > 0.0)) {  // 0, -0.0, negative, NaN: decides nothing
    CHECK(b.lo == -1.0 && b.hi == kInf, "band(%a): {%a, %a}", c.tol2, b.lo, b.hi);
    return;
  }
  const double T = std::sqrt(c.tol2);
  CHECK(b.lo < T && T < b.hi, "band(%a, %a, %a) = {%a, %a} around %a", c.tol2, c.n1max, c.sum_l,
        b.lo, b.hi, T);
  // d and tol_lo as the source defines them
  const double tol_lo = T * (1.0 - 0x1p-50);
  const double d = 0x1p-52 * (6.0 * c.n1max + 8.0 * c.sum_l + 1.0);
  CHECK((b.lo == -1.0) == (d > 0.5 * tol_lo), "band(%a, %a, %a): lo %a, d %a, tol_lo %a", c.tol2,
        c.n1max, c.sum_l, b.lo, d, tol_lo);
}

static void check_band() {
  const double sp[] = {0.0, -0.0, -1.0, -kInf, NAN};
  for (double t2 : sp) {
    const ErrBand b = fabrik_band(t2, 64.0 * 11.0, 8.0);
    CHECK(b.lo == -1.0 && b.hi == kInf, "band(%a): {%a, %a}", t2, b.lo, b.hi);
  }
  Triple list[128];
  const int m = band_list(list);
  CHECK(m >= 30 && m <= 128, "band list of %d", m);
  for (int k = 0; k < m; ++k) check_band_props(list[k]);
  // either side of lo's edge d = tol_lo / 2, for the default launch's d
  const double d = 0x1p-52 * (6.0 * 704.0 + 8.0 * 8.0 + 1.0);
  const double above = 2.0 * d * (1.0 + 1e-9), below = 2.0 * d * (1.0 - 1e-9);
  const Triple ca = {above * above, 704.0, 8.0}, cb = {below * below, 704.0, 8.0};
  check_band_props(ca);
  check_band_props(cb);
  CHECK(fabrik_band(ca.tol2, 704.0, 8.0).lo > 0.0, "T just above 2 d: lo decides");
  CHECK(fabrik_band(cb.tol2, 704.0, 8.0).lo == -1.0, "T just below 2 d: lo decides nothing");
}

// ---- fabrik_qmax -----------------------------------------------------------
static void check_qmax() {
  const struct {
    double L[4], min_abs;
  } cs[] = {{{2, 2, 2, 2}, 2},          {{1, 2, 3, 4}, 1},           {{2, 1, 3, 4}, 1},
            {{3, 2, 1, 4}, 1},          {{4, 3, 2, 1}, 1},           {{-0.5, 5, 7, 9}, 0.5},
            {{5, -0.5, 7, -9}, 0.5},    {{-5, -7, -0.25, -9}, 0.25}, {{-5, 7, -9, -0.125}, 0.125},
            {{-3, -3, -3, -3}, 3},      {{0x1p-100, 1, 1, 1}, 0x1p-100}};
  for (const auto &c : cs) {
    const double q = fabrik_qmax(c.L);
    CHECK(q == std::ldexp(c.min_abs, 382), "qmax{%g, %g, %g, %g} = %a", c.L[0], c.L[1], c.L[2],
          c.L[3], q);
  }
  CHECK(fabrik_qmax(cs[0].L) == 0x1p383, "the default links' qmax");
}

// ---- the plan --------------------------------------------------------------
static const double kTwoPi = 2 * 3.141592653589793;  // 2 * math.pi, as forward.py:23-25 forms it

// The default robot (robot.py: thetas, d, a, alpha rows) on a 256-CU device, a
// fused ordered call of 1M points.
static FabPlanIn base() {
  FabPlanIn in;
  const double dh[16] = {0, 3.141592653589793 / 2, 0, 0, 2, 0, 0, 0,
                         0, 2, 2, 2, 3.141592653589793 / 2, 0, 0, 0};
  std::memcpy(in.dh, dh, sizeof dh);
  for (double &l : in.links) l = 2.0;
  in.n = 1000000;
  in.tol = 1e-3;
  in.max_iter = 100;
  in.variant = 1;
  in.core_req = 2;
  in.bpc_req = 0;
  in.has_table = true;
  in.order_env = 1;
  in.chunk_env = 64;
  in.cus = 256;
  in.ord_ppt = 16;
  in.iter_waves = 2;
  return in;
}

static void check_plan_default() {
  const FabPlan p = fabrik_plan(base());
  CHECK(p.tol2 == tol_threshold(1e-3), "tol2 %a", p.tol2);
  CHECK(p.band_n1 == 64.0 * 11.0, "band_n1 %a", p.band_n1);
  const ErrBand b = fabrik_band(p.tol2, 704.0, 8.0);
  CHECK(p.band.lo == b.lo && p.band.hi == b.hi && b.lo > 0.0, "band {%a, %a}", p.band.lo,
        p.band.hi);
  CHECK(p.qmax == 0x1p383, "qmax %a", p.qmax);
  CHECK(!p.simple && p.ordered && p.core == 2 && !p.refill1 && p.chunk == 64,
        "default: simple %d ordered %d core %d refill1 %d chunk %d", p.simple, p.ordered, p.core,
        p.refill1, p.chunk);
  CHECK(p.grid == 3907 && p.ogrid == 245 && p.pgrid == 512, "default grids %u %u %u", p.grid,
        p.ogrid, p.pgrid);
}

static void check_plan_simple() {
  auto simple = [](const FabPlanIn &in) { return fabrik_plan(in).simple; };
  FabPlanIn in = base();
  CHECK(!simple(in), "the default call is fused");
  for (int v : {0, 1, 2}) {
    in = base();
    in.variant = v;
    CHECK(simple(in) == (v == 0), "variant %d", v);
    CHECK(fabrik_plan(in).refill1 == (v == 2), "variant %d: refill threshold", v);
  }
  for (int mi : {-1, 0, 1}) {
    in = base();
    in.max_iter = mi;
    CHECK(simple(in) == (mi <= 0), "max_iter %d", mi);
  }
  const struct {
    double tol;
    bool simple;
  } tols[] = {{1.0, true}, {std::nextafter(1.0, 0.0), false}, {std::nextafter(1.0, 2.0), true},
              {kInf, true}, {NAN, true}, {0.0, false}, {-1.0, false}, {0.5, false}};
  for (const auto &t : tols) {
    in = base();
    in.tol = t.tol;
    CHECK(simple(in) == t.simple, "tol %a", t.tol);
  }
  // the robot's own angles: theta_2..4 and the four alphas, inclusive +-2 pi
  for (int k : {1, 2, 3, 12, 13, 14, 15})
    for (double sgn : {1.0, -1.0}) {
      in = base();
      in.dh[k] = sgn * kTwoPi;
      CHECK(!simple(in), "dh[%d] = %a is inside", k, in.dh[k]);
      in.dh[k] = sgn * std::nextafter(kTwoPi, kInf);
      CHECK(simple(in), "dh[%d] = %a is outside", k, in.dh[k]);
      in.dh[k] = sgn * kInf;
      CHECK(simple(in), "dh[%d] = %a is outside", k, in.dh[k]);
    }
  in = base();
  in.dh[0] = 100.0;  // theta_1 is replaced by the goal's azimuth
  CHECK(!simple(in), "dh[0] does not count");
  // a simple launch: the grid over n; the chunk field stays 64 whatever the environment
  in = base();
  in.variant = 0;
  in.chunk_env = 17;
  in.n = 257;
  const FabPlan p = fabrik_plan(in);
  CHECK(p.simple && p.grid == 2 && p.chunk == 64 && !p.ordered, "simple launch: grid %u chunk %d",
        p.grid, p.chunk);
}

static void check_plan_ordered() {
  const struct {
    bool table;
    int env;
    int64_t n;
    bool ordered;
  } cs[] = {{true, 1, 1000, true},
            {false, 1, 1000, false},
            {true, 0, 1000, false},
            {true, -1, 1000, true},
            {true, 7, 1000, true},
            {false, 0, 1000, false},
            {true, 1, ((int64_t)1 << 31) - 1, true},
            {true, 1, (int64_t)1 << 31, false},
            {true, 1, (int64_t)1 << 40, false}};
  for (const auto &c : cs) {
    FabPlanIn in = base();
    in.has_table = c.table;
    in.order_env = c.env;
    in.n = c.n;
    const FabPlan p = fabrik_plan(in);
    CHECK(!p.simple && p.ordered == c.ordered, "ordered(table %d, env %d, n %lld) = %d", c.table,
          c.env, (long long)c.n, p.ordered);
  }
  FabPlanIn in = base();
  in.n = ((int64_t)1 << 31) - 1;
  const FabPlan p = fabrik_plan(in);
  CHECK(p.grid == 8388608u && p.ogrid == 524288u && p.pgrid == 512u, "n = 2^31 - 1: %u %u %u",
        p.grid, p.ogrid, p.pgrid);
}

static void check_plan_core() {
  const double in_lo = 0x1p-100, out_lo = std::nextafter(0x1p-100, 0.0);
  const double in_hi = 0x1p100, out_hi = std::nextafter(0x1p100, kInf);
  const struct {
    double L[4];
    int req, core;
  } cs[] = {{{2, 2, 2, 2}, 0, 0},
            {{2, 2, 2, 2}, 1, 1},
            {{2, 2, 2, 2}, 2, 2},
            {{3, 3, 5, 5}, 2, 2},
            {{-2, -2, 2, 2}, 2, 2},
            {{-2, 2, 2, 2}, 2, 1},  // L0 != L1 bitwise, though |L0| == |L1|
            {{2, 3, 2, 2}, 2, 1},
            {{2, 2, 2, 3}, 2, 1},
            {{2, 3, 2, 2}, 1, 1},
            {{2, 3, 2, 2}, 0, 0},
            {{in_lo, in_lo, in_lo, in_lo}, 2, 2},
            {{in_hi, in_hi, in_hi, in_hi}, 2, 2},
            {{-in_lo, -in_lo, -in_hi, -in_hi}, 2, 2},
            {{out_lo, 2, 2, 2}, 2, 0},
            {{2, out_lo, 2, 2}, 1, 0},
            {{2, 2, -out_lo, 2}, 2, 0},
            {{2, 2, 2, out_hi}, 2, 0},
            {{-out_hi, 2, 2, 2}, 1, 0},
            {{2, 2, 0.0, 2}, 2, 0},
            {{2, -0.0, 2, 2}, 1, 0},
            {{2, 2, 2, kInf}, 2, 0},
            {{-kInf, 2, 2, 2}, 2, 0},
            {{2, NAN, 2, 2}, 2, 0},
            {{2, 2, 2, NAN}, 1, 0}};
  for (const auto &c : cs) {
    FabPlanIn in = base();
    std::memcpy(in.links, c.L, sizeof c.L);
    in.core_req = c.req;
    const FabPlan p = fabrik_plan(in);
    CHECK(!p.simple && p.core == c.core, "core(%a, %a, %a, %a; req %d) = %d, want %d", c.L[0],
          c.L[1], c.L[2], c.L[3], c.req, p.core, c.core);
  }
  const double edges[] = {out_lo, in_lo, in_hi, out_hi};
  const bool ok[] = {false, true, true, false};
  for (int k = 0; k < 4; ++k) {
    const double L[4] = {edges[k], edges[k], edges[k], edges[k]};
    CHECK(links_core_ok(L, 4) == ok[k], "links_core_ok(%a)", edges[k]);
  }
}

static void check_plan_chunk() {
  const int cs[][2] = {{0, 64}, {-3, 64}, {65, 64}, {1, 1}, {17, 17}, {64, 64}};
  for (const int *c : cs) {
    FabPlanIn in = base();
    in.chunk_env = c[0];
    CHECK(fabrik_plan(in).chunk == c[1], "chunk(%d) = %d", c[0], fabrik_plan(in).chunk);
  }
}

static void check_plan_grids() {
  // blocks per CU at a size that needs the whole grid: cus * bpc
  const struct {
    int req, waves;
    unsigned pgrid;
  } bs[] = {{0, 2, 512}, {-1, 2, 512}, {1, 2, 256}, {2, 2, 512}, {5, 2, 512},
            {0, 3, 768}, {5, 3, 768}, {2, 3, 512}, {3, 3, 768},  {1, 1, 256}};
  for (const auto &b : bs) {
    FabPlanIn in = base();
    in.bpc_req = b.req;
    in.iter_waves = b.waves;
    CHECK(fabrik_plan(in).pgrid == b.pgrid, "pgrid(bpc_req %d, waves %d) = %u", b.req, b.waves,
          fabrik_plan(in).pgrid);
  }
  // the clamp: cus * bpc unless that is more than ceil(n / 64) / 4 blocks
  const struct {
    int cus, req;
    int64_t n;
    unsigned pgrid, grid;
  } ps[] = {{256, 2, 1, 1, 1},          {256, 2, 63, 1, 1},         {256, 2, 64, 1, 1},
            {256, 2, 65, 1, 1},         {256, 2, 256, 1, 1},        {256, 2, 257, 2, 2},
            {256, 2, 1025, 5, 5},       {256, 2, 130816, 511, 511}, {256, 2, 130817, 512, 512},
            {256, 2, 131071, 512, 512}, {256, 2, 131072, 512, 512}, {256, 2, 131073, 512, 513},
            {256, 1, 65536, 256, 256},  {256, 1, 65280, 255, 255},  {4, 1, 1025, 4, 5},
            {4, 1, 1024, 4, 4},         {4, 1, 960, 4, 4},          {4, 1, 768, 3, 3},
            {304, 0, 1000000, 608, 3907}};
  for (const auto &c : ps) {
    FabPlanIn in = base();
    in.cus = c.cus;
    in.bpc_req = c.req;
    in.n = c.n;
    const FabPlan p = fabrik_plan(in);
    CHECK(p.pgrid == c.pgrid && p.grid == c.grid, "n %lld on %d x %d: pgrid %u grid %u",
          (long long)c.n, c.cus, c.req, p.pgrid, p.grid);
  }
  const struct {
    int ppt;
    int64_t n;
    unsigned ogrid;
  } os[] = {{16, 1, 1}, {16, 4096, 1}, {16, 4097, 2}, {16, 8192, 2}, {8, 4096, 2}, {8, 2049, 2},
            {8, 2048, 1}, {1, 257, 2}};
  for (const auto &c : os) {
    FabPlanIn in = base();
    in.ord_ppt = c.ppt;
    in.n = c.n;
    const FabPlan p = fabrik_plan(in);
    CHECK(p.ordered && p.ogrid == c.ogrid, "ogrid(n %lld, ppt %d) = %u", (long long)c.n, c.ppt,
          p.ogrid);
  }
}

static void check_plan_band_n1() {
  FabPlanIn in = base();
  in.dh[4] = -3.0;  // |d1|
  in.dh[8] = -0.5;  // |a1|
  in.links[1] = -2.0;
  CHECK(fabrik_plan(in).band_n1 == 64.0 * 12.5, "band_n1 %a", fabrik_plan(in).band_n1);
  const double bad[] = {kInf, -kInf, NAN};
  for (double v : bad)
    for (int where = 0; where < 3; ++where) {
      in = base();
      (where == 0 ? in.dh[4] : where == 1 ? in.dh[8] : in.links[2]) = v;
      const FabPlan p = fabrik_plan(in);
      CHECK(p.band_n1 == -1.0, "band_n1 with %a (%d) = %a", v, where, p.band_n1);
    }
  in = base();
  for (double &l : in.links) l = 1e308;  // the sum overflows
  CHECK(fabrik_plan(in).band_n1 == -1.0 && fabrik_plan(in).core == 0, "overflowing links");
}

int main(int argc, char **argv) {
  if (argc > 1 && !std::strcmp(argv[1], "--band")) {
    Triple list[128];
    const int m = band_list(list);
    for (int k = 0; k < m; ++k) {
      const ErrBand b = fabrik_band(list[k].tol2, list[k].n1max, list[k].sum_l);
      std::printf("%a %a %a %a %a\n", list[k].tol2, list[k].n1max, list[k].sum_l, b.lo, b.hi);
    }
    return 0;
  }
  check_tol_threshold();
  check_band();
  check_qmax();
  check_plan_default();
  check_plan_simple();
  check_plan_ordered();
  check_plan_core();
  check_plan_chunk();
  check_plan_grids();
  check_plan_band_n1();
  if (g_fail) {
    std::printf("fabrik_plan_check: %d failures\n", g_fail);
    return 1;
  }
  std::printf("fabrik_plan_check ok (%ld tolerances)\n", g_tols);
  return 0;
}
