// ik_chain.h -- launcher of ik_chain.hip (ik_chain_solve).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ik_chain_row.h"
#include "ik_types.h"

namespace ikhip {

// The table's theta row: the seed of every row when the call has no seed array (by
// value, like ChainParams).
struct ChainHome {
  double th[kChainMaxJoints];
};

// Damped least squares with restarts (ik_chain.hip) of n goals on a chain of nj
// (2..8) joints; pts n x 3, seed n x nj or null (home for every row), ang n x nj;
// iters / tries / fk_err nullable; device pointers.  P.mask != 0 runs the limited
// instantiation.  Stats into S.
void launch_chain_solve(int nj, const ChainParams &P, const ChainHome &home, const double *pts,
                        const double *seed, int64_t n, double tol, int max_iter, double damping,
                        int restarts, double *ang, int32_t *iters, int32_t *tries,
                        double *fk_err, DevStats *S, hipStream_t st);

}  // namespace ikhip
