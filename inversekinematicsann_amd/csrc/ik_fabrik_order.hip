// ik_fabrik_order.hip -- the hard-first work order of a FABRIK ikine solve: the
// launches around ik_fabrik.hip's iteration kernel that turn the context's cost
// table into a queue -> point permutation and fold the call's records back into it.
#include "ik_fabrik_args.h"

namespace ikhip {

// ---------------------------------------------------------- Work order ----
// The persistent iteration kernel hands points out in queue order.  In point
// order a 100-iteration point can be picked up just before the queue runs dry
// and set the launch length alone (≈ 1.4x the lane-iterations / lanes bound
// at 1M random_dist points).  Handing out the expensive points first removes
// most of that tail.  The cost of a point is predicted from its goal cell --
// distance from the shoulder (the seed's first joint) in 64 bins up to the reach
// of links 1..3, and the sine of the elevation in 16 bins -- by the LARGEST
// iteration count the context recorded in that cell on earlier calls (1 point
// in kOrdSample; the old key decays by 1/8 when new records arrive).  The
// largest, not the mean: what sets the tail is a long point starting late, and
// long points (9 % of random_dist points take >= 80 of 100 iterations) sit in
// cells of every mean.  A list-scheduling simulation of 131k lanes on 1M
// reference iteration counts (tol 1e-3 / 1e-5): point order 1.29x / 1.34x the
// lane-iterations / lanes bound, cells by mean 1.15x / 1.23x, cells by sampled
// max 1.04x / 1.03x, exact longest-first 1.01x.  Unseen cells count as hard.
// Costs map to 16 classes; a counting sort (class-major, hardest first; order
// inside a class is whatever the atomics give) yields the queue -> point
// permutation.  Results do not depend on the order: every point is still
// solved by the same arithmetic on its own.
//
// Launches: classify (cell + class per point from the goal alone, class totals)
// -> scatter (class region starts from the totals, one cursor per class: the
// queue -> point permutation) -> iterate (records 1 point in kOrdSample) -> fold
// (one block: this call's records into the table for the next call).
// (kOrdPPT, the points per thread of the classify / scatter blocks: ik_fabrik_args.h)
// (r04: classify and scatter in one launch, the queue in per-class regions of n
// entries: the launch takes 17.8 us against 13.5 + 9.8, but its queue order inside a
// cost class makes the iteration kernel 4 % slower at tol 1e-3 with the same learned
// table; dropped, profiles/r04/ab/fabrik_fused_scatter.txt)
// (r04: spreading a block's class run over its slots -- slot r * 4099 mod run length --
// so that a grab's points come from the whole block: iteration kernel +0.9 %, scatter
// +3 us; profiles/r04/ab/fabrik_order_spread_dropped.txt)

// The shoulder (the seed's first joint, the translation of A_1) is
// (a1 cos t1, a1 sin t1, d1) with t1 the goal's own azimuth: its distance from the
// goal needs no trigonometry.
__device__ __forceinline__ int goal_cell(const RobotDev &r, d3 g) {
  const double rxy = sqrt(g.x * g.x + g.y * g.y) - r.dh[8];
  const double dz = g.z - r.dh[4];
  const double dist = sqrt(rxy * rxy + dz * dz);
  const double reach = r.links[1] + r.links[2] + r.links[3];
  int rb = (int)(dist / reach * kOrdCellsR);
  rb = rb < 0 ? 0 : (rb >= kOrdCellsR ? kOrdCellsR - 1 : rb);
  int eb = dist > 0.0 ? (int)((dz / dist + 1.0) * (0.5 * kOrdCellsE)) : kOrdCellsE / 2;
  eb = eb < 0 ? 0 : (eb >= kOrdCellsE ? kOrdCellsE - 1 : eb);
  return rb * kOrdCellsE + eb;
}

__device__ __forceinline__ int key_class(unsigned int key, int max_iter) {
  // key: 1 + largest recorded iterations, 0 = unseen
  if (key == 0) return kOrdClasses - 1;
  const int k = (int)((long long)(key - 1) * kOrdClasses / (max_iter + 1));
  return k < 0 ? 0 : (k >= kOrdClasses ? kOrdClasses - 1 : k);
}


// Fold ns records into the table: per cell, the largest recorded iteration
// count of the call, or the decayed old key if larger.  One block.
__device__ void order_fold(FabOrderDev *T, unsigned int ns) {
  __shared__ unsigned int lm[kOrdCells];
  const int t = threadIdx.x;
  for (int c = t; c < kOrdCells; c += blockDim.x) lm[c] = 0;
  __syncthreads();
  constexpr int kFoldBatch = 8;  // independent loads in flight
  for (unsigned int k0 = t; k0 < ns; k0 += blockDim.x * kFoldBatch) {
    unsigned int v[kFoldBatch];
#pragma unroll
    for (int j = 0; j < kFoldBatch; ++j) {
      const unsigned int k = k0 + blockDim.x * j;
      v[j] = k < ns ? T->sample[k] : 0xffffffffu;
    }
#pragma unroll
    for (int j = 0; j < kFoldBatch; ++j)
      if (v[j] != 0xffffffffu) atomicMax(&lm[v[j] >> 16], (v[j] & 0xffffu) + 1u);
  }
  __syncthreads();
  for (int c = t; c < kOrdCells; c += blockDim.x) {
    if (lm[c]) {
      const unsigned int old = T->key[c];
      const unsigned int dec = old - (old >> 3);
      T->key[c] = lm[c] > dec ? lm[c] : dec;
    }
  }
}

// 1. classify: the goal's cell and cost class per point (2 bytes), and the
// class totals (one atomic per class and block, into the block's shard: one
// address per class took ~1k same-address atomics per launch at 1M points).
// The cell -> class map of this call is built in LDS first.
__global__ __launch_bounds__(256) void fabrik_classify_kernel(FabArgs a) {
  __shared__ unsigned int cnt[kOrdClasses], unseen;
  __shared__ uint8_t cls[kOrdCells];  // the cell's class, 0xff: unseen (the hardest class)
  const int t = threadIdx.x;
  const int64_t b0 = (int64_t)blockIdx.x * (256 * kOrdPPT);
  d3 g[kOrdPPT];
#pragma unroll
  for (int j = 0; j < kOrdPPT; ++j) {  // all loads in flight before the first use
    const int64_t i = b0 + j * 256 + t;
    if (i < a.n) g[j] = {a.pts[3 * i], a.pts[3 * i + 1], a.pts[3 * i + 2]};
  }
  if (t < kOrdClasses) cnt[t] = 0;
  if (t == 0) unseen = 0;
  // the cell -> class map's table reads, in flight with the goals'
  static_assert(kOrdCells % 256 == 0, "whole table rows per thread");
  unsigned int key[kOrdCells / 256];
#pragma unroll
  for (int q = 0; q < kOrdCells / 256; ++q) key[q] = a.ord->key[t + 256 * q];
#pragma unroll
  for (int q = 0; q < kOrdCells / 256; ++q)
    cls[t + 256 * q] = key[q] ? (uint8_t)key_class(key[q], a.max_iter) : (uint8_t)0xff;
  __syncthreads();
  unsigned int nu = 0;
#pragma unroll
  for (int j = 0; j < kOrdPPT; ++j) {
    const int64_t i = b0 + j * 256 + t;
    if (i < a.n) {
      const int cell = goal_cell(a.r, g[j]);
      int k = cls[cell];
      nu += k == 0xff ? 1u : 0u;
      k = k == 0xff ? kOrdClasses - 1 : k;
      a.cell[i] = (uint16_t)(cell | (k << 10));
      atomicAdd(&cnt[k], 1u);
    }
  }
  // (only the prior's gate reads the count: the first call of a context; a
  // wave sum, then one LDS atomic per wave -- one per thread cost 2 us a launch)
  if (a.prior_gate) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) nu += __shfl_xor(nu, off, 64);
    if ((t & 63) == 0 && nu) atomicAdd(&unseen, nu);
  }
  __syncthreads();
  if (t < kOrdClasses && cnt[t]) atomicAdd(&a.S->cls_tot[t][blockIdx.x % kOrdShards], cnt[t]);
  if (t == 0 && unseen) atomicAdd(&a.S->unseen, (unsigned long long)unseen);
}

// The built-in prior's gate: a table no call has taught yet is
// the prior learned on random_dist batches (ik_fabrik_prior.h).  On a batch of
// another distribution many goals fall in cells it has never seen (uniform box:
// the unreachable far cells; a spring trajectory: the far end of its curve), and
// ordering by it measured slower than point order (r06 lease: uniform box +1.5 %,
// spring +2.3 %).  When more than 1 / kPriorUnseenDiv of the batch lands in unseen
// cells, the first call keeps point order; the call's records then teach the
// table as usual.
constexpr unsigned kPriorUnseenDiv = 50;

// 2. scatter: perm[queue position] = point.  The queue is class-major (hardest
// first), then shard: region (c, s) starts after every harder class and every
// lower shard of class c.  Block b covers the points classify's block b counted
// into shard b % kOrdShards, claims its run inside its region with one atomic
// per class and hands the slots out through LDS atomics.
__global__ __launch_bounds__(256) void fabrik_scatter_kernel(FabArgs a) {
  static_assert(kOrdClasses * kOrdShards == 256, "one total per thread");
  // the prior does not describe this batch (see above): every point in the last
  // class, i.e. the order an empty table gives (block shards, point order inside)
  const bool gated = a.prior_gate && a.S->unseen * kPriorUnseenDiv > (unsigned long long)a.n;
  __shared__ unsigned int cnt[kOrdClasses], base[kOrdClasses];
  __shared__ unsigned int tot[kOrdClasses][kOrdShards], ctot[kOrdClasses];
  const int t = threadIdx.x;
  const int sh = blockIdx.x % kOrdShards;
  if (t < kOrdClasses) cnt[t] = 0;
  // the 256 (class, shard) totals, one load per thread, in flight with the cells
  tot[t / kOrdShards][t % kOrdShards] = (&a.S->cls_tot[0][0])[t];
  const int64_t b0 = (int64_t)blockIdx.x * (256 * kOrdPPT);
  uint16_t cl[kOrdPPT];
#pragma unroll
  for (int j = 0; j < kOrdPPT; ++j) {
    const int64_t i = b0 + j * 256 + t;
    cl[j] = i < a.n ? a.cell[i] : (uint16_t)0xffff;
    if (gated && cl[j] != 0xffff) cl[j] |= (uint16_t)((kOrdClasses - 1) << 10);
  }
  __syncthreads();
  if (gated) {  // (uniform) the shards' totals all in the last class
    unsigned int col = 0;
    if (t < kOrdShards)
      for (int c = 0; c < kOrdClasses; ++c) col += tot[c][t];
    __syncthreads();
    if (t < kOrdShards)
      for (int c = 0; c < kOrdClasses; ++c) tot[c][t] = c == kOrdClasses - 1 ? col : 0u;
    __syncthreads();
  }
#pragma unroll
  for (int j = 0; j < kOrdPPT; ++j)
    if (cl[j] != 0xffff) atomicAdd(&cnt[cl[j] >> 10], 1u);
  if (t < kOrdClasses) {
    unsigned int c = 0;
#pragma unroll
    for (int q = 0; q < kOrdShards; ++q) c += tot[t][q];
    ctot[t] = c;
  }
  __syncthreads();
  if (t < kOrdClasses) {
    // region (t, sh) starts after every harder class and the lower shards of t
    unsigned int start = 0;
    for (int c = kOrdClasses - 1; c > t; --c) start += ctot[c];
    for (int q = 0; q < sh; ++q) start += tot[t][q];
    base[t] = start + (cnt[t] ? atomicAdd(&a.S->cls_cur[t][sh], cnt[t]) : 0u);
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kOrdPPT; ++j) {
    if (cl[j] != 0xffff) {
      const unsigned int pos = atomicAdd(&base[cl[j] >> 10], 1u);
      a.perm[pos] = (int32_t)(b0 + j * 256 + t);
    }
  }
}

// The cost-table fold after an ordered solve (one block): this call's samples
// (the retire steps' stores, published by the kernel boundary) into the table
// the next call's classify reads.
__global__ __launch_bounds__(256) void fabrik_fold_kernel(FabArgs a) {
  const int64_t ns = (a.n + kOrdSample - 1) / kOrdSample;
  order_fold(a.ord, (unsigned int)(ns < kOrdMaxSample ? ns : kOrdMaxSample));
}

void launch_fabrik_order(const FabArgs &a, unsigned grid, hipStream_t stream) {
  kt_begin("fabrik_classify_kernel", stream);
  IK_LAUNCH(fabrik_classify_kernel, dim3(grid), dim3(256), 0, stream, a);
  kt_end(stream);
  kt_begin("fabrik_scatter_kernel", stream);
  IK_LAUNCH(fabrik_scatter_kernel, dim3(grid), dim3(256), 0, stream, a);
  kt_end(stream);
}

void launch_fabrik_fold(const FabArgs &a, hipStream_t stream) {
  kt_begin("fabrik_fold_kernel", stream);
  IK_LAUNCH(fabrik_fold_kernel, dim3(1), dim3(256), 0, stream, a);
  kt_end(stream);
}

}  // namespace ikhip
