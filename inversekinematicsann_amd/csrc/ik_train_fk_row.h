// ik_train_fk_row.h -- one row of the training loss's forward-kinematics term
// (include/ikhip.h "ANN training", ik_ann_train_set_loss): from the last layer's
// scaled outputs a and the scaled inputs x of a row,
//   theta_j = a_j y_scale_j + y_mean_j,  p_k = x_k x_scale_k + x_mean_k,
//   e = FK(wrap(theta)) - p,  e . e  and  J_j . e  (J = dFK / dtheta at wrap(theta)).
// FK and J are the chain of ik_chain_jac.h, shared with ik_refine.hip
// (kinematics/train.py fk_loss_reference restates the row on refine._chain).
// Compiled by the kernel (ik_train.hip train_loss_fk_kernel), which takes the sines
// and cosines from sincos_fk, and by a plain host compiler
// (tests/host/train_fk_row_check.cpp), which takes libm's; everything here is the
// same IEEE operation in the same order (-ffp-contract=off).
#pragma once

#include "ik_chain_jac.h"
#include "ik_train_plan.h"

namespace ikhip {

// wrap(theta) of the row's outputs a (4 floats)
IK_ROW_FN void train_fk_angles(const TrainFkScale &sc, const float *a, double th[4]) {
  for (int j = 0; j < 4; ++j) th[j] = wrap_pi((double)a[j] * sc.ys[j] + sc.ym[j]);
}

struct TrainFkRow {
  double ee;     // e . e
  double je[4];  // J_j . e
};

// jc: {a_i, d_i, cos alpha_i, sin alpha_i} per joint (fk_trip_consts); s, c: the sines
// and cosines of wrap(theta); x: the row's scaled inputs (3 floats).  alpha_ok false
// (some |alpha_i| > 2 pi: FK raises): everything NaN.
IK_ROW_FN TrainFkRow train_fk_row(const double *jc, const TrainFkScale &sc, const double s[4],
                                  const double c[4], const float *xin, bool alpha_ok) {
  const ChainJac f = fk_chain_jac(jc, s, c);
  const RefineJ &J = f.J;
  // what the scaled fp32 input decodes to
  const double px = (double)xin[0] * sc.xs[0] + sc.xm[0];
  const double py = (double)xin[1] * sc.xs[1] + sc.xm[1];
  const double pz = (double)xin[2] * sc.xs[2] + sc.xm[2];
  const double nan = __builtin_nan("");
  const double ex = alpha_ok ? f.x - px : nan, ey = alpha_ok ? f.y - py : nan,
               ez = alpha_ok ? f.z - pz : nan;
  TrainFkRow o;
  o.ee = ex * ex + ey * ey + ez * ez;
  o.je[0] = J.j0x * ex + J.j0y * ey;
  o.je[1] = J.j1x * ex + J.j1y * ey + J.j1z * ez;
  o.je[2] = J.j2x * ex + J.j2y * ey + J.j2z * ez;
  o.je[3] = J.j3x * ex + J.j3y * ey + J.j3z * ez;
  return o;
}

}  // namespace ikhip
