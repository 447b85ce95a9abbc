// ik_train_fk_row.h -- one row of the training loss's forward-kinematics term
// (include/ikhip.h "ANN training", ik_ann_train_set_loss): from the last layer's
// scaled outputs a and the scaled inputs x of a row,
//   theta_j = a_j y_scale_j + y_mean_j,  p_k = x_k x_scale_k + x_mean_k,
//   e = FK(wrap(theta)) - p,  e . e  and  J_j . e  (J = dFK / dtheta at wrap(theta)).
// The chain is ik_refine.hip's, in its operation order: the effector as
// Rz(t1) B1 Rz(t2) B2 Rz(t3) B3 Rz(t4) B4 e4 applied right to left to a vector, the
// four Jacobian columns riding along (kinematics/train.py fk_loss_reference restates
// it on refine._chain).  Compiled by the kernel (ik_train.hip train_loss_fk_kernel),
// which takes the sines and cosines from sincos_fk, and by a plain host compiler
// (tests/host/train_fk_row_check.cpp), which takes libm's; everything here is the
// same IEEE operation in the same order (-ffp-contract=off).
#pragma once

#include <math.h>

#include "ik_train_plan.h"

#if defined(__HIPCC__)
#define IK_ROW_FN __host__ __device__ inline
#else
#define IK_ROW_FN inline
#endif

namespace ikhip {

// theta - 2 pi rint(theta / 2 pi), as ik_refine wraps: sincos_fk is valid on
// [-2 pi, 2 pi] only, and FK is periodic
IK_ROW_FN double train_fk_wrap(double t) {
  const double two_pi = 2 * 3.141592653589793;
  return t - two_pi * rint(t / two_pi);
}

// wrap(theta) of the row's outputs a (4 floats)
IK_ROW_FN void train_fk_angles(const TrainFkScale &sc, const float *a, double th[4]) {
  for (int j = 0; j < 4; ++j) th[j] = train_fk_wrap((double)a[j] * sc.ys[j] + sc.ym[j]);
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
  const double a1 = jc[0], d1 = jc[1], ca1 = jc[2], sa1 = jc[3];
  const double a2 = jc[4], d2 = jc[5], ca2 = jc[6], sa2 = jc[7];
  const double a3 = jc[8], d3 = jc[9], ca3 = jc[10], sa3 = jc[11];
  const double a4 = jc[12], d4 = jc[13];
  const double s0 = s[0], c0 = c[0], s1 = s[1], c1 = c[1], s2 = s[2], c2 = c[2], s3 = s[3],
               c3 = c[3];
  // ---- joint 4: v = B4 e4 = (a4, 0, d4); Rz(t4)
  double x = a4, y = 0.0, z = d4;
  double xr = c3 * x - s3 * y, yr = s3 * x + c3 * y;
  double j3x = -yr, j3y = xr, j3z = 0.0;  // column 4
  x = xr;
  y = yr;
  // B3, then its rotation on the open column
  double yb = ca3 * y - sa3 * z, zb = sa3 * y + ca3 * z + d3;
  x = x + a3;
  y = yb;
  z = zb;
  double wy = ca3 * j3y - sa3 * j3z, wz = sa3 * j3y + ca3 * j3z;
  j3y = wy;
  j3z = wz;
  // ---- joint 3: Rz(t3)
  xr = c2 * x - s2 * y;
  yr = s2 * x + c2 * y;
  double j2x = -yr, j2y = xr, j2z = 0.0;  // column 3
  x = xr;
  y = yr;
  double wx = c2 * j3x - s2 * j3y;
  wy = s2 * j3x + c2 * j3y;
  j3x = wx;
  j3y = wy;
  // B2
  yb = ca2 * y - sa2 * z;
  zb = sa2 * y + ca2 * z + d2;
  x = x + a2;
  y = yb;
  z = zb;
  wy = ca2 * j3y - sa2 * j3z;
  wz = sa2 * j3y + ca2 * j3z;
  j3y = wy;
  j3z = wz;
  wy = ca2 * j2y - sa2 * j2z;
  wz = sa2 * j2y + ca2 * j2z;
  j2y = wy;
  j2z = wz;
  // ---- joint 2: Rz(t2)
  xr = c1 * x - s1 * y;
  yr = s1 * x + c1 * y;
  double j1x = -yr, j1y = xr, j1z = 0.0;  // column 2
  x = xr;
  y = yr;
  wx = c1 * j3x - s1 * j3y;
  wy = s1 * j3x + c1 * j3y;
  j3x = wx;
  j3y = wy;
  wx = c1 * j2x - s1 * j2y;
  wy = s1 * j2x + c1 * j2y;
  j2x = wx;
  j2y = wy;
  // B1
  yb = ca1 * y - sa1 * z;
  zb = sa1 * y + ca1 * z + d1;
  x = x + a1;
  y = yb;
  z = zb;
  wy = ca1 * j3y - sa1 * j3z;
  wz = sa1 * j3y + ca1 * j3z;
  j3y = wy;
  j3z = wz;
  wy = ca1 * j2y - sa1 * j2z;
  wz = sa1 * j2y + ca1 * j2z;
  j2y = wy;
  j2z = wz;
  wy = ca1 * j1y - sa1 * j1z;
  wz = sa1 * j1y + ca1 * j1z;
  j1y = wy;
  j1z = wz;
  // ---- joint 1: Rz(t1)
  xr = c0 * x - s0 * y;
  yr = s0 * x + c0 * y;
  const double j0x = -yr, j0y = xr;  // column 1 (its z is 0)
  x = xr;
  y = yr;
  wx = c0 * j3x - s0 * j3y;
  wy = s0 * j3x + c0 * j3y;
  j3x = wx;
  j3y = wy;
  wx = c0 * j2x - s0 * j2y;
  wy = s0 * j2x + c0 * j2y;
  j2x = wx;
  j2y = wy;
  wx = c0 * j1x - s0 * j1y;
  wy = s0 * j1x + c0 * j1y;
  j1x = wx;
  j1y = wy;

  // what the scaled fp32 input decodes to
  const double px = (double)xin[0] * sc.xs[0] + sc.xm[0];
  const double py = (double)xin[1] * sc.xs[1] + sc.xm[1];
  const double pz = (double)xin[2] * sc.xs[2] + sc.xm[2];
  const double nan = __builtin_nan("");
  const double ex = alpha_ok ? x - px : nan, ey = alpha_ok ? y - py : nan,
               ez = alpha_ok ? z - pz : nan;
  TrainFkRow o;
  o.ee = ex * ex + ey * ey + ez * ez;
  o.je[0] = j0x * ex + j0y * ey;
  o.je[1] = j1x * ex + j1y * ey + j1z * ez;
  o.je[2] = j2x * ex + j2y * ey + j2z * ez;
  o.je[3] = j3x * ex + j3y * ey + j3z * ez;
  return o;
}

}  // namespace ikhip
