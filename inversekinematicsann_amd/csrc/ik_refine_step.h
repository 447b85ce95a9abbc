// ik_refine_step.h -- the linear algebra of one damped-least-squares step of
// ik_refine, with and without joint limits (include/ikhip.h "Refine" and "Joint
// limits" state the arithmetic; kinematics/refine.py restates it in numpy).
// Compiled by the kernel (ik_refine.hip) and by a plain host compiler
// (tests/host/refine_limits_check.cpp): every operation is the same IEEE operation
// in the same order (-ffp-contract=off), so both give the same bits.  J (RefineJ)
// comes from the chain of ik_chain_jac.h, which is held to the same contract.
//
// refine_solve: A = J' J'^T + lambda^2 I (3 x 3, six entries), LDL^T without
// pivoting, delta = J'^T A^-1 e, where J' is J with the columns of the lock mask
// replaced by +0.0.  The replacement is a select, not a product: a locked column
// adds only +0.0 terms to sums that are written once, in one order, so an empty
// mask gives the free refine's bits.
//
// refine_step: the active-set loop of the limited refine.  A limited joint that
// sits on a bound and whose delta points out of the interval is locked and the
// system solved again; locks only grow, so there are at most four re-solves.  On
// the device the loop is wave-uniform: it runs while any lane has a new lock, and a
// lane with nothing new solves the same system again and gets the same values.
#pragma once

#include "ik_chain_jac.h"

#if defined(__HIP_DEVICE_COMPILE__)
#define IK_REFINE_ANY(p) __any(p)
#else
#define IK_REFINE_ANY(p) (p)
#endif

namespace ikhip {

// The robot's joint limits as the kernels take them (by value: wave-uniform).
// Bit i of mask: joint i is limited, lo[i] <= hi[i] both inside [-pi, pi]; a free
// joint holds -inf / +inf.
struct JointLimits {
  double lo[4], hi[4];
  unsigned mask;
};

// t pulled into [lo, hi]; a NaN stays NaN.
IK_ROW_FN double refine_project(double t, double lo, double hi) {
  t = t < lo ? lo : t;
  return t > hi ? hi : t;
}

// d[0..3] = J'^T (J' J'^T + lam2 I)^-1 e, J' = J without the columns in `lock`.
IK_ROW_FN void refine_solve(const RefineJ &J, double ex, double ey, double ez, double lam2,
                            unsigned lock, double d[4]) {
  const double j0x = (lock & 1u) ? 0.0 : J.j0x, j0y = (lock & 1u) ? 0.0 : J.j0y;
  const double j1x = (lock & 2u) ? 0.0 : J.j1x, j1y = (lock & 2u) ? 0.0 : J.j1y,
               j1z = (lock & 2u) ? 0.0 : J.j1z;
  const double j2x = (lock & 4u) ? 0.0 : J.j2x, j2y = (lock & 4u) ? 0.0 : J.j2y,
               j2z = (lock & 4u) ? 0.0 : J.j2z;
  const double j3x = (lock & 8u) ? 0.0 : J.j3x, j3y = (lock & 8u) ? 0.0 : J.j3y,
               j3z = (lock & 8u) ? 0.0 : J.j3z;
  // A = J J^T + lambda^2 I (rows x, y, z; column 1 has no z part)
  const double A00 = j0x * j0x + j1x * j1x + j2x * j2x + j3x * j3x + lam2;
  const double A10 = j0y * j0x + j1y * j1x + j2y * j2x + j3y * j3x;
  const double A11 = j0y * j0y + j1y * j1y + j2y * j2y + j3y * j3y + lam2;
  const double A20 = j1z * j1x + j2z * j2x + j3z * j3x;
  const double A21 = j1z * j1y + j2z * j2y + j3z * j3y;
  const double A22 = j1z * j1z + j2z * j2z + j3z * j3z + lam2;
  // LDL^T, no pivoting (A is SPD)
  const double l10 = A10 / A00, l20 = A20 / A00;
  const double D1 = A11 - l10 * A10;
  const double u21 = A21 - l20 * A10;
  const double l21 = u21 / D1;
  const double D2 = A22 - l20 * A20 - l21 * u21;
  const double y1 = ey - l10 * ex;
  const double y2 = ez - l20 * ex - l21 * y1;
  const double q2 = y2 / D2;
  const double q1 = y1 / D1 - l21 * q2;
  const double q0 = ex / A00 - l10 * q1 - l20 * q2;
  // delta = J^T q
  d[0] = j0x * q0 + j0y * q1;
  d[1] = j1x * q0 + j1y * q1 + j1z * q2;
  d[2] = j2x * q0 + j2y * q1 + j2z * q2;
  d[3] = j3x * q0 + j3y * q1 + j3z * q2;
}

// The limited joints outside `lock` that sit on a bound with delta pointing out.
IK_ROW_FN unsigned refine_new_locks(const double t[4], const double d[4], const JointLimits &L,
                                    unsigned lock) {
  unsigned nw = 0;
  for (int i = 0; i < 4; ++i) {
    const bool out = ((t[i] <= L.lo[i]) & (d[i] < 0.0)) | ((t[i] >= L.hi[i]) & (d[i] > 0.0));
    nw |= (out ? 1u : 0u) << i;
  }
  return nw & L.mask & ~lock;
}

// One step's delta under the limits L at the angles t (inside the limits); returns
// the lock mask the delta was solved with.  resolves (nullable): solves after the
// first that changed this row's mask.
IK_ROW_FN unsigned refine_step(const RefineJ &J, double ex, double ey, double ez, double lam2,
                               const double t[4], const JointLimits &L, double d[4],
                               int *resolves) {
  unsigned lock = 0;
  int rs = 0;
  for (;;) {
    refine_solve(J, ex, ey, ez, lam2, lock, d);
    const unsigned nw = refine_new_locks(t, d, L, lock);
    lock |= nw;
    rs += nw != 0;
    if (!IK_REFINE_ANY(nw != 0)) break;
  }
  if (resolves) *resolves = rs;
  return lock;
}

}  // namespace ikhip
