// ik_refine.h -- launchers of ik_refine.hip.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ik_refine_step.h"
#include "ik_types.h"

namespace ikhip {

struct RobotConstDev;  // ik_fk_chain.h

// Damped-least-squares refine (ik_refine.hip) of seed angles (n x 4, float64 or
// the ANN's float32) towards pts; rc: the robot's constants (device).  iters /
// fk_err nullable; iteration and FK-error stats into S.  jl: the robot's joint
// limits (ik_refine_step.h); with no limited joint the kernel without them runs.
void launch_refine(const RobotConstDev *rc, const double *pts, const double *seed, int64_t n,
                   double tol, int max_iter, double damping, double *ang, int32_t *iters,
                   double *fk_err, bool check_limits, const JointLimits &jl, DevStats *S,
                   hipStream_t st);
void launch_refine_f32(const RobotConstDev *rc, const double *pts, const float *seed, int64_t n,
                       double tol, int max_iter, double damping, double *ang, int32_t *iters,
                       double *fk_err, bool check_limits, const JointLimits &jl, DevStats *S,
                       hipStream_t st);
// ik_check_joint_limits: rows of ang (n x 4, device) with a limited joint's wrapped
// angle outside [lo, hi]: the lowest into S's first error, their count into n_capped.
void launch_check_joint_limits(const JointLimits &jl, const double *ang, int64_t n, DevStats *S,
                               hipStream_t st);

}  // namespace ikhip
