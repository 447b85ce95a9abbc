// ik_analytic.h -- launcher of ik_analytic.hip.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ik_types.h"

namespace ikhip {

struct RobotConstDev;  // ik_fk_chain.h

// Closed-form solve (ik_analytic.hip) of a yaw + planar 3R robot (the host checks
// it: ik_analytic_plan.h) for pts, the pitches (nullable: the goal's own
// elevation) and the elbow branch -1 / +1; nearest: an infeasible pitch moves to
// the nearest feasible one.  pitch_out / fk_err nullable; moved rows count as
// n_capped in S, failed rows report IK_E_OUT_OF_REACH.
void launch_analytic(const RobotConstDev *rc, const double *pts, const double *pitch, int64_t n,
                     int elbow, bool nearest, double *ang, double *pitch_out, double *fk_err,
                     bool check_limits, DevStats *S, hipStream_t st);

}  // namespace ikhip
