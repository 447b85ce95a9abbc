// ik_fk.h -- launchers of ik_fk.hip: the per-context kernels (stats reset,
// workspace check, robot constants) and forward kinematics.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ik_launch.h"
#include "ik_types.h"

namespace ikhip {

struct RobotConstDev;  // ik_fk_chain.h

void launch_reset_stats(DevStats *S, hipStream_t st);
void launch_check_limits(const RobotDev &r, const double *pts, int64_t n, DevStats *S,
                         hipStream_t st);
void launch_fk(const RobotDev &r, const double *ang, int64_t n, double *xyz, double *mats,
               DevStats *S, hipStream_t st);
// FK of a chain of nj (2..kFkMaxJoints) joints; dh: device 4 x nj, mats nullable
// n x nj x 16 (2..8 unrolled, longer chains a run-time joint loop).
constexpr int kFkMaxJoints = 1024;
void launch_fk_n(int nj, const double *dh, const double *ang, int64_t n, double *xyz,
                 double *mats, DevStats *S, hipStream_t st);
// Per-robot seed constants (RobotConstDev) into device memory, on stream st.
void launch_robot_const(const RobotDev &r, RobotConstDev *rc, hipStream_t st);

}  // namespace ikhip
