// train_plan_check.cpp -- CPU check of csrc/ik_train_plan.cpp, built with
// -fsanitize=address,undefined by tests/test_train_plan_cpu.py and run directly.
//
// Everything is checked by what it has to be, never by a copy of the plan's code:
// the two block layouts as lists of (offset, floats needed) in the documented order
// -- aligned, large enough, disjoint, inside the total; an epoch's steps and chunks
// as a partition of the rows; the losses on sums whose answer is known; Adam's
// step size at the ends of its range; each refusal by its text.
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/ikhip.h"
#include "ik_train_plan.h"

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

static_assert(sizeof(float) == sizeof(int32_t), "perm is carved in floats");

// ---- layouts ---------------------------------------------------------------
struct Part {
  const char *name;
  size_t off, need;  // floats
};

// `parts` in the documented order: each on a multiple of 64 floats, ending before the
// next begins (so: large enough, disjoint, in order), the last inside the total.
static void check_parts(const char *what, const std::vector<Part> &parts, size_t total) {
  CHECK(parts[0].off == 0, "%s: %s starts at %zu", what, parts[0].name, parts[0].off);
  for (size_t i = 0; i < parts.size(); ++i) {
    const Part &p = parts[i];
    const size_t end = i + 1 < parts.size() ? parts[i + 1].off : total;
    CHECK(p.off % 64 == 0, "%s: %s at %zu is not a multiple of 64", what, p.name, p.off);
    CHECK(p.off <= end && p.need <= end - p.off, "%s: %s at %zu needs %zu floats, ends at %zu",
          what, p.name, p.off, p.need, end);
  }
  CHECK(total <= SIZE_MAX / sizeof(float), "%s: %zu floats overflow size_t in bytes", what, total);
}

static void check_state(const std::vector<int32_t> &dims, int max_batch) {
  const int n = (int)dims.size() - 1;
  const TrainStateLayout L = train_state_layout(n, dims.data(), max_batch);
  char what[96];
  std::snprintf(what, sizeof(what), "state %d layers (%d .. %d) batch %d", n, dims[0], dims[n],
                max_batch);
  int widest = 0;
  for (int32_t d : dims) widest = d > widest ? d : widest;
  CHECK(L.widest == widest, "%s: widest %d, not %d", what, L.widest, widest);
  std::vector<Part> parts;
  const size_t mb = (size_t)max_batch;
  for (int l = 0; l < n; ++l) {
    const size_t kn = (size_t)dims[l] * (size_t)dims[l + 1], o = (size_t)dims[l + 1];
    parts.push_back({"W", L.W[l], kn}), parts.push_back({"mW", L.mW[l], kn});
    parts.push_back({"vW", L.vW[l], kn}), parts.push_back({"gW", L.gW[l], kn});
    parts.push_back({"b", L.b[l], o}), parts.push_back({"mb", L.mb[l], o});
    parts.push_back({"vb", L.vb[l], o}), parts.push_back({"gb", L.gb[l], o});
  }
  for (int l = 0; l <= n; ++l) parts.push_back({"A", L.A[l], mb * (size_t)dims[l]});
  parts.push_back({"y", L.y, mb * (size_t)dims[n]});
  parts.push_back({"dZ0", L.dZ[0], mb * (size_t)widest});
  parts.push_back({"dZ1", L.dZ[1], mb * (size_t)widest});
  check_parts(what, parts, L.total);
}

static void check_data(int64_t n_train, int64_t n_val, int d0, int dL) {
  const TrainDataLayout D = train_data_layout(n_train, n_val, d0, dL);
  char what[96];
  std::snprintf(what, sizeof(what), "data %lld + %lld rows of %d / %d", (long long)n_train,
                (long long)n_val, d0, dL);
  const size_t nt = (size_t)n_train, nv = (size_t)n_val;
  check_parts(what,
              {{"X", D.X, nt * d0}, {"Xs", D.Xs, nt * d0}, {"Y", D.Y, nt * dL},
               {"Ys", D.Ys, nt * dL}, {"Xv", D.Xv, nv * d0}, {"Yv", D.Yv, nv * dL},
               {"perm", D.perm, nt}},
              D.total);
  if (n_val == 0)
    CHECK(D.Xv == D.Yv && D.Yv == D.perm, "%s: validation parts of %zu and %zu floats", what,
          D.Yv - D.Xv, D.perm - D.Yv);
}

static void check_layouts() {
  std::vector<std::pair<std::vector<int32_t>, int>> shapes;
  std::vector<int32_t> ref = {3};
  ref.insert(ref.end(), 12, 500);
  ref.push_back(4);
  shapes.push_back({ref, 32});                                      // the reference network
  shapes.push_back({{3, 33, 4}, 1});
  shapes.push_back({{5, 48, 48, 2}, 40});
  shapes.push_back({std::vector<int32_t>(kTrainMaxLayers + 1, kTrainMaxWidth), kTrainMaxBatch});
  shapes.push_back({{1, 63, 64, 65}, 3});
  shapes.push_back({{65, 64, 63, 1}, 65});
  for (int32_t w : {1, 63, 64, 65})
    for (int mb : {1, 63, 64, 65}) shapes.push_back({{w, w}, mb});
  for (const auto &s : shapes) {
    check_state(s.first, s.second);
    const int d0 = s.first.front(), dL = s.first.back();
    for (int64_t nt : {(int64_t)1, (int64_t)13, (int64_t)64, (int64_t)65, (int64_t)1372,
                       (int64_t)INT32_MAX})
      for (int64_t nv : {(int64_t)0, (int64_t)1, (int64_t)19, (int64_t)676, (int64_t)INT32_MAX})
        check_data(nt, nv, d0, dL);
  }
}

// ---- the epoch plan ----------------------------------------------------------
// `count` pieces of at most `cap` rows partition 0..n: contiguous from row 0, every
// piece 1..cap rows, only the last short.
template <class Row, class Rows>
static void check_partition(const char *what, int64_t n, int cap, int64_t count, Row row,
                            Rows rows) {
  int64_t at = 0;
  for (int64_t i = 0; i < count; ++i) {
    CHECK(row(i) == at, "%s of %lld by %d: piece %lld starts at %lld, not %lld", what,
          (long long)n, cap, (long long)i, (long long)row(i), (long long)at);
    const int r = rows(i);
    CHECK(r >= 1 && r <= cap && (r == cap || i == count - 1),
          "%s of %lld by %d: piece %lld of %lld has %d rows", what, (long long)n, cap,
          (long long)i, (long long)count, r);
    at += r;
  }
  CHECK(at == n, "%s of %lld by %d: the pieces hold %lld rows", what, (long long)n, cap,
        (long long)at);
}

static void check_epoch_plan() {
  long cases = 0;
  for (int64_t nt = 1; nt <= 70; ++nt)
    for (int batch = 1; batch <= 9; ++batch)
      for (int64_t nv : {0, 1, 7, 8, 9, 19})
        for (int mb : {8, 9}) {
          const TrainEpoch e = train_epoch(nt, nv, batch, mb);
          check_partition("steps", nt, batch, e.steps, [&](int64_t s) { return e.step_row(s); },
                          [&](int64_t s) { return e.step_rows(s); });
          check_partition("chunks", nv, mb, e.vchunks, [&](int64_t v) { return e.chunk_row(v); },
                          [&](int64_t v) { return e.chunk_rows(v); });
          CHECK(e.slots() == e.steps + e.vchunks, "slots %lld", (long long)e.slots());
          // every step's and every chunk's sum is rows * dL * c: both losses are c, to
          // within the roundings of the mean (one per slot's term and add, a few more)
          for (int dL : {1, 4})
            for (double c : {0.3, 1.7}) {
              std::vector<double> sums;
              for (int64_t s = 0; s < e.steps; ++s) sums.push_back(e.step_rows(s) * dL * c);
              for (int64_t v = 0; v < e.vchunks; ++v) sums.push_back(e.chunk_rows(v) * dL * c);
              double tl = -1.0, vl = -1.0;
              train_epoch_losses(e, dL, sums.data(), &tl, &vl);
              CHECK(std::fabs(tl - c) <= (2.0 * e.steps + 8.0) * DBL_EPSILON * c,
                    "%lld by %d: constant loss %g came out %.17g", (long long)nt, batch, c, tl);
              if (nv == 0)
                CHECK(std::isnan(vl), "no validation rows: val loss %g", vl);
              else
                CHECK(std::fabs(vl - c) <= (2.0 * e.vchunks + 8.0) * DBL_EPSILON * c,
                      "%lld by %d: constant val loss %g came out %.17g", (long long)nv, mb, c, vl);
            }
          ++cases;
        }
  CHECK(cases == 70 * 9 * 6 * 2, "the sweep ran %ld cases", cases);
}

// Unequal steps: the step losses sums[s] / (rows_s dL) weighted by rows_s / n_train
// are sum(sums) / (n_train dL) -- not the plain mean of the step losses.  Cases of
// at most 6 steps: the plan rounds each term twice (rows dL is exact), each add once
// and the last division once, (steps + 2) * 2^-53 <= 8.9e-16 relative for positive
// sums, inside the 1e-15 this holds it to; long double carries 11 bits more.
static void check_weighting() {
  const int cs[][4] = {{13, 19, 5, 8}, {7, 1, 3, 8}, {33, 9, 8, 8}, {6, 0, 5, 9}, {50, 70, 9, 9}};
  uint64_t x = 88172645463325252ull;
  for (const auto &c : cs)
    for (int dL : {1, 3, 4}) {
      const TrainEpoch e = train_epoch(c[0], c[1], c[2], c[3]);
      CHECK(e.steps <= 6, "%d by %d: %lld steps", c[0], c[2], (long long)e.steps);
      std::vector<double> sums;
      long double ts = 0.0L, vs = 0.0L;
      double plain = 0.0;
      for (int64_t i = 0; i < e.slots(); ++i) {
        x ^= x << 13, x ^= x >> 7, x ^= x << 17;  // xorshift64
        sums.push_back(0.01 + (double)(x >> 11) * 0x1p-53 * 40.0);
        (i < e.steps ? ts : vs) += (long double)sums.back();
        if (i < e.steps) plain += sums.back() / (e.step_rows(i) * dL) / e.steps;
      }
      const long double want_t = ts / ((long double)c[0] * dL);
      double tl = -1.0, vl = -1.0;
      train_epoch_losses(e, dL, sums.data(), &tl, &vl);
      CHECK(std::fabs((double)((long double)tl - want_t)) <= 1e-15 * (double)want_t,
            "%d by %d, dL %d: loss %.17g, by rows %.17Lg", c[0], c[2], dL, tl, want_t);
      if (e.step_rows(e.steps - 1) != c[2])  // (a short last step: the plain mean is another number)
        CHECK(std::fabs(plain - (double)want_t) > 1e-6 * (double)want_t, "%d by %d: a blunt case",
              c[0], c[2]);
      if (c[1] > 0) {
        const long double want_v = vs / ((long double)c[1] * dL);
        CHECK(std::fabs((double)((long double)vl - want_v)) <= 1e-15 * (double)want_v,
              "%d by %d, dL %d: val loss %.17g, want %.17Lg", c[1], c[3], dL, vl, want_v);
      } else {
        CHECK(std::isnan(vl), "no validation rows: val loss %g", vl);
      }
    }
}

// ---- Adam ---------------------------------------------------------------------
static void check_adam() {
  const double lr = 1e-3, b1 = 0.9, b2 = 0.999, eps = 1e-7;
  AdamDev a = train_adam(lr, b1, b2, eps, 1);
  CHECK(a.alpha == (float)(lr * std::sqrt(1.0 - b2) / (1.0 - b1)), "alpha_1 = %a", a.alpha);
  CHECK(a.b1 == b1 && a.b2 == b2 && a.omb1 == 1.0 - b1 && a.omb2 == 1.0 - b2,
        "betas %a %a %a %a", a.b1, a.omb1, a.b2, a.omb2);
  CHECK(a.eps == (float)eps, "eps %a", a.eps);
  // beta^t -> 0: alpha_t -> lr (0.999^10000 = e^-10.005, 0.999^100000 < 2^-53)
  a = train_adam(lr, b1, b2, eps, 10000);
  CHECK(std::fabs((double)a.alpha / lr - 1.0) < 1e-4, "alpha_10000 = %a", a.alpha);
  a = train_adam(lr, b1, b2, eps, 100000);
  CHECK(a.alpha == (float)lr, "alpha_100000 = %a", a.alpha);
  for (int64_t t : {1, 2, 1000}) {  // beta = 0: plain RMS scaling, alpha_t = lr
    a = train_adam(lr, 0.0, 0.0, 0.0, t);
    CHECK(a.alpha == (float)lr && a.omb1 == 1.0 && a.omb2 == 1.0 && a.b1 == 0.0 && a.b2 == 0.0 &&
              a.eps == 0.0f,
          "beta 0, t %lld: alpha %a", (long long)t, a.alpha);
  }
}

// ---- refusals -----------------------------------------------------------------
struct Begin {
  int n_layers = 2;
  std::vector<int32_t> dims = {3, 8, 4}, acts = {IK_ACT_TANH, IK_ACT_LINEAR};
  float w = 0.0f;
  std::vector<const float *> W = {&w, &w}, b = {&w, &w};
  int max_batch = 8;
  double lr = 1e-3, beta1 = 0.9, beta2 = 0.999, eps = 1e-7;
  std::string why() const {
    return train_begin_refusal(n_layers, dims.data(), acts.data(), W.data(), b.data(), max_batch,
                               lr, beta1, beta2, eps);
  }
};

static void expect(const std::string &got, const char *want, const char *what) {
  CHECK(got == want, "%s: '%s', expected '%s'", what, got.c_str(), want);
}

static void check_refusals() {
  Begin ok;
  expect(ok.why(), "", "a plain begin");
  expect(train_begin_refusal(2, nullptr, ok.acts.data(), ok.W.data(), ok.b.data(), 8, 1e-3, 0.9,
                             0.999, 1e-7), "NULL argument", "dims NULL");
  expect(train_begin_refusal(2, ok.dims.data(), nullptr, ok.W.data(), ok.b.data(), 8, 1e-3, 0.9,
                             0.999, 1e-7), "NULL argument", "acts NULL");
  expect(train_begin_refusal(2, ok.dims.data(), ok.acts.data(), nullptr, ok.b.data(), 8, 1e-3, 0.9,
                             0.999, 1e-7), "NULL argument", "W NULL");
  expect(train_begin_refusal(2, ok.dims.data(), ok.acts.data(), ok.W.data(), nullptr, 8, 1e-3, 0.9,
                             0.999, 1e-7), "NULL argument", "b NULL");
  for (int n : {0, -1, kTrainMaxLayers + 1}) {
    Begin g;
    g.n_layers = n;
    expect(g.why(), "n_layers must be 1..24", "n_layers");
  }
  for (int32_t d : {0, -3, kTrainMaxWidth + 1}) {
    Begin g;
    g.dims[2] = d;
    expect(g.why(), "dims[2] must be 1..1024", "a width");
    g.dims[0] = d;  // the first one is named
    expect(g.why(), "dims[0] must be 1..1024", "the input width");
  }
  for (int32_t a : {-1, IK_ACT_SIGMOID + 1}) {
    Begin g;
    g.acts[1] = a;
    expect(g.why(), "unknown activation", "an activation code");
  }
  for (int which : {0, 1}) {
    Begin g;
    (which ? g.W : g.b)[1] = nullptr;
    expect(g.why(), "NULL layer weights", "a layer's pointer");
  }
  for (int mb : {0, -8, kTrainMaxBatch + 1}) {
    Begin g;
    g.max_batch = mb;
    expect(g.why(), "max_batch must be 1..4096", "max_batch");
  }
  const double bad_lr[] = {0.0, -1e-3, NAN, INFINITY}, bad_beta[] = {1.0, -0.1, 1.5, NAN},
               bad_eps[] = {-1e-7, NAN, INFINITY};
  for (double v : bad_lr) {
    Begin g;
    g.lr = v;
    expect(g.why(), "bad Adam parameters", "lr");
  }
  for (double v : bad_beta) {
    Begin g, h;
    g.beta1 = v, h.beta2 = v;
    expect(g.why(), "bad Adam parameters", "beta1");
    expect(h.why(), "bad Adam parameters", "beta2");
  }
  for (double v : bad_eps) {
    Begin g;
    g.eps = v;
    expect(g.why(), "bad Adam parameters", "eps");
  }
  {  // the largest legal arguments
    Begin g;
    g.n_layers = kTrainMaxLayers;
    g.dims.assign(kTrainMaxLayers + 1, kTrainMaxWidth);
    g.acts.assign(kTrainMaxLayers, IK_ACT_SIGMOID);
    g.W.assign(kTrainMaxLayers, &g.w), g.b.assign(kTrainMaxLayers, &g.w);
    g.max_batch = kTrainMaxBatch;
    g.lr = DBL_MAX, g.beta1 = g.beta2 = std::nextafter(1.0, 0.0), g.eps = DBL_MAX;
    expect(g.why(), "", "the caps");
    g.beta1 = g.beta2 = 0.0, g.eps = 0.0, g.lr = DBL_TRUE_MIN;
    expect(g.why(), "", "beta 0, eps 0");
  }

  const int64_t big = (int64_t)INT32_MAX + 1;
  expect(train_data_refusal(1, 0), "", "one training row");
  expect(train_data_refusal(INT32_MAX, INT32_MAX), "", "the most rows");
  for (int64_t nt : {(int64_t)0, (int64_t)-1, big})
    expect(train_data_refusal(nt, 0), "bad args", "n_train");
  for (int64_t nv : {(int64_t)-1, big}) expect(train_data_refusal(5, nv), "bad args", "n_val");

  std::vector<int32_t> perm(16);
  for (int i = 0; i < 16; ++i) perm[i] = 15 - i;
  expect(train_epoch_refusal(nullptr, 16, 8, 8), "", "data order");
  expect(train_epoch_refusal(perm.data(), 16, 8, 8), "", "a permutation");
  expect(train_epoch_refusal(perm.data(), 16, 1, 8), "", "batch 1");
  expect(train_epoch_refusal(nullptr, 16, 0, 8), "batch 0 outside 1..max_batch 8", "batch 0");
  expect(train_epoch_refusal(perm.data(), 16, 9, 8), "batch 9 outside 1..max_batch 8", "batch 9");
  perm[3] = -1, perm[7] = 16;
  expect(train_epoch_refusal(perm.data(), 16, 8, 8), "perm[3] = -1 outside 0..15", "perm -1");
  perm[3] = 12;
  expect(train_epoch_refusal(perm.data(), 16, 8, 8), "perm[7] = 16 outside 0..15", "perm 16");
  perm[7] = 15;
  expect(train_epoch_refusal(perm.data(), 16, 8, 8), "", "the largest entry");
}

int main() {
  check_layouts();
  check_epoch_plan();
  check_weighting();
  check_adam();
  check_refusals();
  if (g_fail) {
    std::printf("train_plan_check: %d checks failed\n", g_fail);
    return 1;
  }
  std::printf("train_plan_check ok\n");
  return 0;
}
