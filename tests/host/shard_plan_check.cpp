// shard_plan_check.cpp -- CPU check of csrc/ik_shard_plan.cpp, built with
// -fsanitize=address,undefined by tests/test_shard_plan_cpu.py.
//
// Every expected value is worked out here by brute force (loops over the chunks,
// sorted expansions of the histograms), never by the code under test.  The
// histograms are allocated with exactly IK_FKHIST_BINS counts, so a read past
// them is a sanitizer report.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "ik_shard_plan.h"

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

static int64_t min64(int64_t a, int64_t b) { return a < b ? a : b; }

static void check_plan(int64_t n, int g, int C) {
  CHECK(plan_args_ok(n, g, C), "plan_args_ok(%lld, %d, %d)", (long long)n, g, C);
  ik_shard_plan P;
  std::memset(&P, 0xEE, sizeof(P));
  make_plan(n, g, C, &P);
  const int64_t cg = (int64_t)C * g;
  const int64_t S = n / cg + (n % cg != 0);  // ceil(n / (C g))
  int chunks = 0;
  int64_t full = 0;
  for (int c = 0; c < C; ++c) {
    if ((int64_t)c * g * S < n) ++chunks;                 // the chunk holds rows
    if ((int64_t)(c + 1) * g * S <= n) full += g * S;     // ... all of its g S
  }
  CHECK(P.n == n && P.nranks == g, "plan (%lld, %d, %d): n / nranks", (long long)n, g, C);
  CHECK(P.part_rows == S, "plan (%lld, %d, %d): part_rows %lld, want %lld", (long long)n, g, C,
        (long long)P.part_rows, (long long)S);
  CHECK(P.chunks == chunks, "plan (%lld, %d, %d): chunks %d, want %d", (long long)n, g, C,
        P.chunks, chunks);
  CHECK(P.full_rows == full, "plan (%lld, %d, %d): full_rows %lld, want %lld", (long long)n, g, C,
        (long long)P.full_rows, (long long)full);
  // the parts in (c, r) order tile [0, n): each starts where the last ended
  std::vector<unsigned char> seen(n <= 5000 ? (size_t)n : 0, 0);
  int64_t at = 0;
  for (int c = 0; c < C; ++c)
    for (int r = 0; r < g; ++r) {
      int64_t b = -7, e = -7;
      part_of(P, r, c, &b, &e);
      const int64_t i = (int64_t)c * g + r;
      CHECK(b == min64(i * S, n) && e == min64((i + 1) * S, n),
            "part (%lld, %d, %d) c %d r %d: [%lld, %lld)", (long long)n, g, C, c, r, (long long)b,
            (long long)e);
      CHECK(b == at && e >= b, "part (%lld, %d, %d) c %d r %d: starts at %lld, the last ended at %lld",
            (long long)n, g, C, c, r, (long long)b, (long long)at);
      if ((int64_t)(c + 1) * g * S <= P.full_rows)
        CHECK(e - b == S, "part (%lld, %d, %d) c %d r %d: %lld rows of a whole chunk",
              (long long)n, g, C, c, r, (long long)(e - b));
      if (c >= P.chunks) CHECK(e == b, "part (%lld, %d, %d) c %d r %d: rows past the plan's chunks",
                               (long long)n, g, C, c, r);
      for (int64_t k = b < 0 ? 0 : b; k < e && k < (int64_t)seen.size(); ++k) ++seen[(size_t)k];
      at = e;
    }
  CHECK(at == n, "plan (%lld, %d, %d): the parts end at %lld", (long long)n, g, C, (long long)at);
  for (size_t k = 0; k < seen.size(); ++k)
    CHECK(seen[k] == 1, "plan (%lld, %d, %d): row %zu in %d parts", (long long)n, g, C, k, seen[k]);
}

static void check_plans() {
  const int64_t ns[] = {0, 1, 2, 7, 257, 258, 4999, 5000, ((int64_t)1 << 48) - 1};
  const int gs[] = {1, 2, 3, 8, 1024};
  for (int64_t n : ns)
    for (int g : gs)
      for (int C = 1; C <= 8; ++C) check_plan(n, g, C);
  CHECK(!plan_args_ok(-1, 2, 1), "n = -1");
  CHECK(!plan_args_ok((int64_t)1 << 48, 2, 1), "n = 2^48");
  CHECK(plan_args_ok(((int64_t)1 << 48) - 1, 2, 1), "n = 2^48 - 1");
  CHECK(!plan_args_ok(10, 0, 1) && !plan_args_ok(10, 1025, 1), "nranks 0 / 1025");
  CHECK(plan_args_ok(10, 1, 1) && plan_args_ok(10, 1024, 1), "nranks 1 / 1024");
  CHECK(!plan_args_ok(10, 2, 0) && !plan_args_ok(10, 2, 9), "chunks 0 / 9");
  CHECK(plan_args_ok(10, 2, 1) && plan_args_ok(10, 2, 8), "chunks 1 / 8");
}

static ik_shard_tail tail(int64_t oob, int64_t err, int code, int max_it, int64_t sum_it,
                          int64_t capped, double max_fk, double sum_fk, int64_t rows) {
  ik_shard_tail t;
  std::memset(&t, 0, sizeof(t));
  t.first_oob = oob;
  t.first_err = err;
  t.first_err_code = code;
  t.max_iters = max_it;
  t.sum_iters = sum_it;
  t.n_capped = capped;
  t.max_fk_err = max_fk;
  t.sum_fk_err = sum_fk;
  t.rows = rows;
  return t;
}

// The expected reduction: the failing indices sorted, the rest added up in rank order.
static void check_reduce(const std::vector<ik_shard_tail> &t, const char *what) {
  ik_stats s;
  std::memset(&s, 0xEE, sizeof(s));
  tail_reduce(t.data(), (int)t.size(), &s);
  std::vector<int64_t> oob;
  std::vector<std::pair<int64_t, int>> err;
  int max_it = 0;
  int64_t sum_it = 0, capped = 0;
  double max_fk = 0.0, sum_fk = 0.0;
  for (const ik_shard_tail &x : t) {
    if (x.first_oob >= 0) oob.push_back(x.first_oob);
    if (x.first_err >= 0) err.push_back({x.first_err, x.first_err_code});
    max_it = std::max(max_it, x.max_iters);
    sum_it += x.sum_iters;
    capped += x.n_capped;
    max_fk = std::max(max_fk, x.max_fk_err);
    sum_fk += x.sum_fk_err;
  }
  std::sort(oob.begin(), oob.end());
  std::sort(err.begin(), err.end());
  CHECK(s.first_oob == (oob.empty() ? -1 : oob[0]), "%s: first_oob %lld", what, (long long)s.first_oob);
  CHECK(s.first_err == (err.empty() ? -1 : err[0].first), "%s: first_err %lld", what,
        (long long)s.first_err);
  CHECK(s.first_err_code == (err.empty() ? IK_OK : err[0].second), "%s: first_err_code %d", what,
        s.first_err_code);
  CHECK(s.max_iters == max_it && s.sum_iters == sum_it && s.n_capped == capped,
        "%s: iteration stats", what);
  CHECK(s.max_fk_err == max_fk && s.sum_fk_err == sum_fk, "%s: FK-error stats", what);
  CHECK(s.gather_ms == 0.0, "%s: gather_ms %g", what, s.gather_ms);
}

static void check_tails() {
  // the lowest index is on the middle rank (FK errors), the last rank (reach)
  check_reduce({tail(900, 70, IK_E_DOMAIN, 12, 1000, 1, 0.5, 10.0, 100),
                tail(-1, 40, IK_E_ZERODIV, 100, 2000, 3, 0.25, 20.5, 100),
                tail(300, -1, IK_OK, 7, 300, 0, 0.75, 0.125, 98)},
               "three ranks");
  check_reduce({tail(-1, -1, IK_OK, 3, 30, 0, 1e-9, 1e-7, 10), tail(-1, -1, IK_OK, 4, 41, 0, 2e-9, 3e-7, 10)},
               "no failure");
  check_reduce({tail(5, 0, IK_E_ANGLE_RANGE, 9, 90, 2, 0.0, 0.0, 0), tail(0, 6, IK_E_ZERODIV, 1, 1, 0, 3.0, 3.0, 1)},
               "index 0 wins");
  // one rank: its own tail, field for field
  const ik_shard_tail one = tail(17, 4, IK_E_ZERODIV, 55, 12345, 6, 0.375, 99.5, 1000);
  check_reduce({one}, "one rank");
  ik_stats s;
  tail_reduce(&one, 1, &s);
  CHECK(s.first_oob == 17 && s.first_err == 4 && s.first_err_code == IK_E_ZERODIV &&
            s.max_iters == 55 && s.sum_iters == 12345 && s.n_capped == 6 &&
            s.max_fk_err == 0.375 && s.sum_fk_err == 99.5,
        "one rank gives back its own tail");
  const ik_shard_tail none = tail(-1, -1, IK_OK, 0, 0, 0, 0.0, 0.0, 0);
  tail_reduce(&none, 1, &s);
  CHECK(s.first_oob == -1 && s.first_err == -1 && s.first_err_code == IK_OK, "all -1 stays -1");
}

// dist.py hist_quantile's closed form: 16 bins per octave from 2^-64.
static double edge(int b) {
  if (b >= IK_FKHIST_BINS - 1) return HUGE_VAL;
  return (1.0 + (double)(b % 16 + 1) / 16.0) * std::pow(2.0, b / 16 - 64);
}

static void check_edges() {
  const double two64 = 18446744073709551616.0;
  CHECK(fkhist_upper(-1) == 0.0, "upper(-1) %g", fkhist_upper(-1));
  CHECK(fkhist_upper(0) == 1.0625 / two64, "upper(0) %g", fkhist_upper(0));
  CHECK(fkhist_upper(15) == 2.0 / two64, "upper(15) %g", fkhist_upper(15));
  CHECK(fkhist_upper(16) == 2.125 / two64, "upper(16) %g", fkhist_upper(16));
  CHECK(fkhist_upper(2046) == 1.9375 * (two64 / 2.0), "upper(2046) %g", fkhist_upper(2046));
  CHECK(fkhist_upper(2047) == HUGE_VAL, "upper(2047) %g", fkhist_upper(2047));
  for (int b : {0, 15, 16, 2046, 2047}) CHECK(fkhist_upper(b) == edge(b), "upper(%d) != edge", b);
}

using Hist = std::vector<uint32_t>;
static Hist hist(std::initializer_list<std::pair<int, uint32_t>> bins) {
  Hist h(IK_FKHIST_BINS, 0u);
  for (const auto &b : bins) h[(size_t)b.first] = b.second;
  return h;
}

static void check_quantiles(const std::vector<Hist> &hs, const char *what) {
  std::vector<const uint32_t *> p;
  std::vector<int> bins;  // one entry per counted error: its bin
  for (const Hist &h : hs) {
    p.push_back(h.data());
    for (int b = 0; b < IK_FKHIST_BINS; ++b) bins.insert(bins.end(), h[(size_t)b], b);
  }
  std::sort(bins.begin(), bins.end());
  const size_t m = bins.size();
  for (double q : {0.5, 0.99, 1.0, 1e-12}) {
    const double got = fkhist_quantile(p.data(), (int)p.size(), q);
    if (m == 0) {
      CHECK(std::isnan(got), "%s q %g: %g for no counted error", what, q, got);
      continue;
    }
    const size_t k = std::max<size_t>(1, (size_t)std::ceil(q * (double)m));  // the k-th smallest
    CHECK(got == edge(bins[k - 1]), "%s q %g: %g, want %g (bin %d)", what, q, got,
          edge(bins[k - 1]), bins[k - 1]);
  }
}

int main() {
  check_plans();
  check_tails();
  check_edges();
  check_quantiles({hist({{3, 2}, {10, 1}, {100, 5}})}, "one rank");
  check_quantiles({hist({{0, 1}})}, "one error");
  check_quantiles({hist({{700, 4}, {701, 1}}), hist({}), hist({{5, 3}, {700, 2}, {2047, 1}})},
                  "three ranks");
  check_quantiles({hist({{900, 99}}), hist({{901, 1}}), hist({{899, 100}})}, "three ranks, p99");
  check_quantiles({hist({})}, "one empty rank");
  check_quantiles({hist({}), hist({}), hist({})}, "three empty ranks");
  if (g_fail) {
    std::printf("shard_plan_check: %d failure(s)\n", g_fail);
    return 1;
  }
  std::printf("shard_plan_check ok\n");
  return 0;
}
