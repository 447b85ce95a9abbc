// ik_chain_jac.h -- the forward-kinematics chain with its Jacobian, the one copy the
// refine (ik_refine.hip) and the training loss's FK term (ik_train_fk_row.h) share:
// the effector Rz(t1) B1 Rz(t2) B2 Rz(t3) B3 Rz(t4) B4 e4 of fk_error_cs (ik_fk_chain.h),
// B_i = Tz(d_i) Tx(a_i) Rx(alpha_i), applied right to left to a vector, with the four
// Jacobian columns riding along -- d Rz(t_i) v / dt_i = (-y', x', 0) of the rotated
// (x', y'), then only the rotations to its left.  Compiled by the kernels, which take
// the sines and cosines from sincos_fk, and by a plain host compiler
// (tests/host/chain_jac_check.cpp), which is given them; kinematics/refine.py _chain_cs
// restates it operation for operation.
#pragma once

#include "ik_row.h"

namespace ikhip {

// The Jacobian's columns (column 1 has no z part).
struct RefineJ {
  double j0x, j0y;
  double j1x, j1y, j1z;
  double j2x, j2y, j2z;
  double j3x, j3y, j3z;
};

struct ChainJac {
  double x, y, z;  // the effector
  RefineJ J;
};

// jc: {a_i, d_i, cos alpha_i, sin alpha_i} per joint (fk_trip_consts; 14 entries are
// read); s, c: the sines and cosines of the four angles.  Written out joint by joint:
// as a loop over the joints (_chain_cs's form) it gives the same bits and registers,
// but another instruction schedule, with which the limited refine kernel measured
// about 1 % slower on the MI355X.
IK_ROW_FN ChainJac fk_chain_jac(const double *jc, const double s[4], const double c[4]) {
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
  return {x, y, z, {j0x, j0y, j1x, j1y, j1z, j2x, j2y, j2z, j3x, j3y, j3z}};
}

}  // namespace ikhip
