// ik_stats.h -- device helpers that report into the call's DevStats: the first
// error, the workspace check and the wave / block reductions of the batch stats.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ik_types.h"

namespace ikhip {

// ------------------------------------------------------------- stats ----
__device__ __forceinline__ void record_error(DevStats *S, int64_t idx, int code) {
  unsigned long long key = ((unsigned long long)idx << 8) | (unsigned long long)code;
  atomicMin(&S->first_err_key, key);
}

__device__ __forceinline__ bool outside(const double *lim, double x, double y, double z) {
  // kinematics/inverse.py:26-35: inclusive bounds, dict order x, y, z
  return (x < lim[0] || x > lim[1]) || (y < lim[2] || y > lim[3]) || (z < lim[4] || z > lim[5]);
}

// 64-lane wave sum of a 64-bit value.
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__device__ __forceinline__ int wave_max_i32(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off, 64));
  return v;
}

__device__ __forceinline__ double wave_max_f64(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
  return v;
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// Block-wide FABRIK iteration stats (blockDim 256): one atomic per counter per
// block, into the block's shard.  Every thread of the block must call it.
// s / c / m: this thread's iteration sum, capped-point count and largest count.
__device__ __forceinline__ void block_iter_stats_acc(DevStats *S, unsigned long long s,
                                                     unsigned long long c, int m) {
  __shared__ unsigned long long red_s[4], red_c[4];
  __shared__ int red_m[4];
  s = wave_sum_u64(s);
  c = wave_sum_u64(c);
  m = wave_max_i32(m);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    red_s[w] = s;
    red_c[w] = c;
    red_m[w] = m;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int nw = (blockDim.x + 63) >> 6;
    for (int i = 1; i < nw; ++i) {
      s += red_s[i];
      c += red_c[i];
      m = max(m, red_m[i]);
    }
    const int sh = blockIdx.x % kStatShards;
    if (s) atomicAdd(&S->sum_iters[sh], s);
    if (c) atomicAdd(&S->n_capped[sh], c);
    if (m) atomicMax(&S->max_iters[sh], m);
  }
}

__device__ __forceinline__ void block_iter_stats(DevStats *S, bool valid, int it, int max_iter) {
  block_iter_stats_acc(S, valid ? (unsigned long long)it : 0ull,
                       (valid && it >= max_iter) ? 1ull : 0ull, valid ? it : 0);
}

// FK round-trip error stats: one atomic pair per wave into the block's shard.
// mx / sm: this lane's largest and summed finite errors.  The whole wave calls it.
__device__ __forceinline__ void wave_fk_stats(DevStats *S, double mx, double sm) {
  mx = wave_max_f64(mx);
  sm = wave_sum_f64(sm);
  if ((threadIdx.x & 63) == 0) {
    const int sh = blockIdx.x % kStatShards;
    atomicMax(&S->max_fk_err_bits[sh], (unsigned long long)__double_as_longlong(mx));
    atomicAdd(&S->sum_fk_err[sh], sm);
  }
}

}  // namespace ikhip
