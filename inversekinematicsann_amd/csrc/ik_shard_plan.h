// ik_shard_plan.h -- the arithmetic of a sharded call that every rank must agree
// on (ik_shard.hip): the chunk plan and a rank's parts, the reduction of the
// gathered tails, the FK-error histogram's bin edges and its quantiles.  Plain
// C++, no HIP header and no context: the code is tested on the CPU
// (tests/test_shard_plan_cpu.py).
#pragma once

#include "../../include/ikhip.h"

namespace ikhip {

bool plan_args_ok(int64_t n, int nranks, int chunks);
// S = ceil(n / (C g)); the chunks that hold rows; the rows of the full ones.
void make_plan(int64_t n, int g, int C, ik_shard_plan *p);
// Rank r's rows [*b, *e) of chunk c: [(c g + r) S, (c g + r + 1) S) clipped to n.
void part_of(const ik_shard_plan &p, int r, int c, int64_t *b, int64_t *e);
// Rank order, as one process would meet the points: the lowest global failing
// index wins, sums add up, FK-error max over ranks.
void tail_reduce(const ik_shard_tail *t, int nranks, ik_stats *s);
// The upper edge of a histogram bin (fkhist_bin, ik_types.h): 0 below the
// first, HUGE_VAL from the last.
double fkhist_upper(int bin);
// The upper edge of the bin holding the ceil(q m)-th smallest of the m errors
// counted in the ranks' histograms (IK_FKHIST_BINS counts each); NaN for m = 0.
double fkhist_quantile(const uint32_t *const *hists, int nranks, double q);

}  // namespace ikhip
