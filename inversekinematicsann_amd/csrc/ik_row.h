// ik_row.h -- what the row headers share (ik_chain_jac.h, ik_refine_step.h,
// ik_train_fk_row.h, ik_analytic_row.h): functions that a kernel and a plain host
// compiler both compile, every operation the same IEEE operation in the same order
// (-ffp-contract=off), so both give the same bits.  Needs no HIP header.
#pragma once

#include <math.h>

#if defined(__HIPCC__)
#define IK_ROW_FN __host__ __device__ inline
#else
#define IK_ROW_FN inline
#endif

namespace ikhip {

// theta - 2 pi rint(theta / 2 pi): in [-pi, pi] (exact for |theta| <= 8 pi).
// sincos_fk is valid on [-2 pi, 2 pi] only, and FK is periodic.
IK_ROW_FN double wrap_pi(double t) {
  const double two_pi = 2 * 3.141592653589793;
  return t - two_pi * rint(t / two_pi);
}

}  // namespace ikhip
