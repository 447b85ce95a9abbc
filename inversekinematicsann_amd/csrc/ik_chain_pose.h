// ik_chain_pose.h -- launcher of ik_chain_pose.hip (ik_chain_pose_solve).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ik_chain.h"
#include "ik_types.h"

namespace ikhip {

// Damped least squares on position and orientation with restarts (ik_chain_pose.hip)
// of n pose goals on a chain of nj (2..8) joints; pts n x 3, rot n x 9 (row-major
// 3 x 3), seed n x nj or null (home for every row), ang n x nj; iters / tries / fk_err /
// rot_err nullable; device pointers.  P.mask != 0 runs the limited instantiation.
// Stats into S.
void launch_chain_pose_solve(int nj, const ChainParams &P, const ChainHome &home,
                             const double *pts, const double *rot, const double *seed, int64_t n,
                             double tol, double rot_tol, double rot_weight, int max_iter,
                             double damping, int restarts, double *ang, int32_t *iters,
                             int32_t *tries, double *fk_err, double *rot_err, DevStats *S,
                             hipStream_t st);

}  // namespace ikhip
