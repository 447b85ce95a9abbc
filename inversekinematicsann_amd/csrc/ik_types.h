// ik_types.h -- the types every kernel family shares: the call's device stats
// block, a 3-vector and the FK-error histogram's bin.  The public interface
// (ikhip.h: the IK_* codes) comes in through here.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ikhip.h"

namespace ikhip {

constexpr double kPi = 3.141592653589793;  // math.pi

// Device-side accumulators of one call (reset by reset_stats_kernel).  The
// batch sums are sharded: each workgroup reduces in registers/LDS and adds to
// shard blockIdx % kStatShards, so no single word takes more than a few
// hundred atomics per launch; the host folds the shards.
constexpr int kStatShards = 64;
constexpr int kOrdClasses = 16;  // FABRIK work-order cost classes (queue order: hardest first)
constexpr int kOrdShards = 16;   // ... and the counter shards per class (blocks b % kOrdShards)
// Work-queue heads of the persistent FABRIK kernel: one returning device-scope
// atomicAdd on a single word saturates near 88 grabs/us (MI355X_MICROARCH.md,
// "dequeue"), which 2048 waves grabbing 64-point chunks reach; a head per XCD
// (blocks b % 8 share one) divides that contention by 8.
constexpr int kQueueHeads = 8;
struct DevStats {
  unsigned long long first_oob;      // atomicMin of point index
  unsigned long long first_err_key;  // atomicMin of (index << 8) | code
  unsigned long long unseen;         // FABRIK classify: points whose goal cell the cost table has not seen
  // FABRIK work order: points per (cost class, block shard), and the scatter's
  // cursor inside each (class, shard) region of the queue
  unsigned int cls_tot[kOrdClasses][kOrdShards];
  unsigned int cls_cur[kOrdClasses][kOrdShards];
  unsigned long long sum_iters[kStatShards];
  unsigned long long n_capped[kStatShards];
  unsigned long long max_fk_err_bits[kStatShards];  // atomicMax on non-negative double bits
  double sum_fk_err[kStatShards];
  int max_iters[kStatShards];
  // the FABRIK iteration kernel's work queue: kQueueHeads heads, one 128-B line
  // each, head h handing out the queue's chunks h, h + kQueueHeads, ...
  alignas(128) unsigned long long heads[kQueueHeads][16];
};

struct d3 {
  double x, y, z;
};

// The FK-error histogram bin of e (ikhip.h IK_FKHIST_BINS): 16 bins per octave
// from the float64 exponent and top 4 mantissa bits, monotonic in e; -1 for NaN,
// inf and negative values (not counted, like the max / sum stats).
__host__ __device__ inline int fkhist_bin(double e) {
  if (!(e >= 0.0) || e > 1.7976931348623157e308) return -1;
  uint64_t b;
  __builtin_memcpy(&b, &e, sizeof(b));
  b &= 0x7fffffffffffffffull;
  const int k = ((int)(b >> 52) - (1023 - 64)) * 16 + (int)((b >> 48) & 15);
  return k < 0 ? 0 : (k >= IK_FKHIST_BINS ? IK_FKHIST_BINS - 1 : k);
}

}  // namespace ikhip
