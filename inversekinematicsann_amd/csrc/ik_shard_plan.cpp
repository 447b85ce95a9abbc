// ik_shard_plan.cpp -- see ik_shard_plan.h.  Host only (HOSTCXX).
#include "ik_shard_plan.h"

#include <cmath>
#include <cstring>

namespace ikhip {

bool plan_args_ok(int64_t n, int nranks, int chunks) {
  return n >= 0 && n < ((int64_t)1 << 48) && nranks >= 1 && nranks <= 1024 && chunks >= 1 &&
         chunks <= IK_MAX_GATHER_CHUNKS;
}

void make_plan(int64_t n, int g, int C, ik_shard_plan *p) {
  std::memset(p, 0, sizeof(*p));
  p->n = n;
  p->nranks = g;
  const int64_t cg = (int64_t)C * g;
  p->part_rows = n > 0 ? (n + cg - 1) / cg : 0;
  const int64_t per_chunk = p->part_rows * g;
  p->chunks = n > 0 ? (int)((n + per_chunk - 1) / per_chunk) : 0;
  p->full_rows = per_chunk > 0 ? (n / per_chunk) * per_chunk : 0;
}

void part_of(const ik_shard_plan &p, int r, int c, int64_t *b, int64_t *e) {
  const int64_t S = p.part_rows;
  const int64_t lo = ((int64_t)c * p.nranks + r) * S, hi = lo + S;
  *b = lo < p.n ? lo : p.n;
  *e = hi < p.n ? hi : p.n;
}

void tail_reduce(const ik_shard_tail *t, int nranks, ik_stats *s) {
  std::memset(s, 0, sizeof(*s));
  s->first_oob = -1;
  s->first_err = -1;
  s->first_err_code = IK_OK;
  for (int r = 0; r < nranks; ++r) {
    if (t[r].first_oob >= 0 && (s->first_oob < 0 || t[r].first_oob < s->first_oob))
      s->first_oob = t[r].first_oob;
    if (t[r].first_err >= 0 && (s->first_err < 0 || t[r].first_err < s->first_err)) {
      s->first_err = t[r].first_err;
      s->first_err_code = t[r].first_err_code;
    }
    s->max_iters = t[r].max_iters > s->max_iters ? t[r].max_iters : s->max_iters;
    s->sum_iters += t[r].sum_iters;
    s->n_capped += t[r].n_capped;
    s->max_fk_err = t[r].max_fk_err > s->max_fk_err ? t[r].max_fk_err : s->max_fk_err;
    s->sum_fk_err += t[r].sum_fk_err;
  }
}

double fkhist_upper(int bin) {
  if (bin < 0 || bin >= IK_FKHIST_BINS - 1) return bin < 0 ? 0.0 : HUGE_VAL;
  return std::ldexp(1.0 + (double)(bin % 16 + 1) / 16.0, bin / 16 - 64);
}

double fkhist_quantile(const uint32_t *const *hists, int nranks, double q) {
  uint64_t tot = 0;
  for (int r = 0; r < nranks; ++r)
    for (int b = 0; b < IK_FKHIST_BINS; ++b) tot += hists[r][b];
  if (tot == 0) return NAN;
  const uint64_t want = (uint64_t)std::ceil(q * (double)tot);
  uint64_t cum = 0;
  for (int b = 0; b < IK_FKHIST_BINS; ++b) {
    for (int r = 0; r < nranks; ++r) cum += hists[r][b];
    if (cum >= (want ? want : 1)) return fkhist_upper(b);
  }
  return NAN;
}

}  // namespace ikhip
