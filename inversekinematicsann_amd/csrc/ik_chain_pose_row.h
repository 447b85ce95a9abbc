// ik_chain_pose_row.h -- one row of ik_chain_pose_solve (include/ikhip.h "Chain pose
// solve"): ik_chain_row.h's chain with the tool frame and the joint axes riding along,
// the two rotation errors, and the 6-row damped least-squares solve with a lock mask
// and its active-set step.  The position, the three linear rows, the scaling, the
// placing, the new locks and the start points are ik_chain_row.h's own functions, so
// with rot_weight = 0 every value that reaches the angles is ik_chain_solve's, bit for
// bit.  Compiled by the kernel (ik_chain_pose.hip) and by a plain host compiler
// (tests/host/chain_pose_row_check.cpp), -ffp-contract=off in both;
// kinematics/chain.py restates it in numpy.  Needs no HIP header.
#pragma once

#include "ik_chain_row.h"

namespace ikhip {

// chain_jac's effector and linear columns, the tool frame R (r[k]: column k, in the
// base frame) and the joint axes (wx[0], wy[0], wz[0] are identically 0, 0, 1).
template <int NJ>
struct PoseJacN {
  ChainJacN<NJ> lin;
  double r[3][3];
  double wx[NJ], wy[NJ], wz[NJ];
};

// chain_jac<NJ> itself for the position and the linear columns, then its loop once
// more, right to left, for the passengers that take the rotations and no translation:
// the three direction vectors that start as the columns of Rx(alpha_NJ) and end as the
// columns of R, and axis i, opened as (0, 0, 1) when joint i is reached (Rz(t_i) leaves
// it alone), which then takes only the rotations to its left, as linear column i does.
template <int NJ>
IK_ROW_FN PoseJacN<NJ> pose_jac(const double (*jc)[4], const double *s, const double *c) {
  PoseJacN<NJ> f;
  f.lin = chain_jac<NJ>(jc, s, c);
  const double can = jc[NJ - 1][2], san = jc[NJ - 1][3];
  f.r[0][0] = 1.0, f.r[0][1] = 0.0, f.r[0][2] = 0.0;
  f.r[1][0] = 0.0, f.r[1][1] = can, f.r[1][2] = san;
  f.r[2][0] = 0.0, f.r[2][1] = -san, f.r[2][2] = can;
#pragma unroll
  for (int i = NJ - 1; i >= 0; --i) {
    const double ci = c[i], si = s[i];
#pragma unroll
    for (int k = 0; k < 3; ++k) {  // Rz(t_i) on the frame
      const double vx = ci * f.r[k][0] - si * f.r[k][1], vy = si * f.r[k][0] + ci * f.r[k][1];
      f.r[k][0] = vx;
      f.r[k][1] = vy;
    }
#pragma unroll
    for (int k = i + 1; k < NJ; ++k) {  // ... and on the axes to its right
      const double vx = ci * f.wx[k] - si * f.wy[k], vy = si * f.wx[k] + ci * f.wy[k];
      f.wx[k] = vx;
      f.wy[k] = vy;
    }
    f.wx[i] = 0.0;
    f.wy[i] = 0.0;
    f.wz[i] = 1.0;
    if (i > 0) {  // Rx(alpha_i) (1-based) of B_i; the translations move no direction
      const double ca = jc[i - 1][2], sa = jc[i - 1][3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double vy = ca * f.r[k][1] - sa * f.r[k][2], vz = sa * f.r[k][1] + ca * f.r[k][2];
        f.r[k][1] = vy;
        f.r[k][2] = vz;
      }
#pragma unroll
      for (int k = i; k < NJ; ++k) {
        const double vy = ca * f.wy[k] - sa * f.wz[k], vz = sa * f.wy[k] + ca * f.wz[k];
        f.wy[k] = vy;
        f.wz[k] = vz;
      }
    }
  }
  return f;
}

// e_w = 1/2 sum_k r_k x g_k (r_k, g_k: the columns of R and of the goal G, row-major):
// sin(phi) axis in the base frame.  Each entry is ((k = 0) + (k = 1)) + (k = 2), a
// term being r_a g_b - r_b g_a, then times 0.5.
IK_ROW_FN void pose_rot_step_error(const double (*r)[3], const double *G, double *ew) {
#pragma unroll
  for (int m = 0; m < 3; ++m) {
    const int a = (m + 1) % 3, b = (m + 2) % 3;
    double acc = r[0][a] * G[3 * b] - r[0][b] * G[3 * a];
#pragma unroll
    for (int k = 1; k < 3; ++k) acc = acc + (r[k][a] * G[3 * b + k] - r[k][b] * G[3 * a + k]);
    ew[m] = 0.5 * acc;
  }
}

// er = sqrt(1/2 sum_ij (R_ij - G_ij)^2), the sum row-major from (0, 0): 2 sin(phi / 2)
// for an orthonormal G.  The stop rule's error: at phi = pi e_w is zero and er is 2.
IK_ROW_FN double pose_rot_error(const double (*r)[3], const double *G) {
  double acc = 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double v = r[j][i] - G[3 * i + j];
      acc = (i == 0 && j == 0) ? v * v : acc + v * v;
    }
  return sqrt(0.5 * acc);
}

// d[0..NJ-1] = J'^T (J' J'^T + lam2 I)^-1 e' for the 6 x NJ matrix J' whose rows 0..2
// are the linear ones and rows 3..5 w times the axes, the columns in `lock` replaced by
// +0.0 (a select), e' = (e, w e_w) as the caller formed it.  A_ij = sum_k J'_ik J'_jk
// over the joints in joint order from joint 1's term (row 2, whose joint-1 entry is
// identically zero: from joint 2's, as chain_solve), lam2 added last on the diagonal.
// LDL^T without pivoting:
//   u_ij = A_ij - sum_{k<j} l_ik u_jk (k ascending; u_jj = D_j), l_ij = u_ij / D_j
//   y_i = e'_i - sum_{k<i} l_ik y_k
//   q_i = y_i / D_i - sum_{k>i} l_ki q_k (k ascending)
//   d_k = sum_r J'_rk q_r (r ascending; joint 1 without r = 2)
// With w = 0 every rotational term is an exact zero and d is chain_solve's (the zero
// delta of a locked joint, a sum of zero products, may differ in sign).
template <int NJ>
IK_ROW_FN void pose_solve(const PoseJacN<NJ> &f, const double *e, double w, double lam2,
                          unsigned lock, double *d) {
  double J[6][NJ];
#pragma unroll
  for (int k = 0; k < NJ; ++k) {
    const bool l = (lock >> k) & 1u;
    J[0][k] = l ? 0.0 : f.lin.jx[k];
    J[1][k] = l ? 0.0 : f.lin.jy[k];
    J[2][k] = l ? 0.0 : f.lin.jz[k];
    J[3][k] = l ? 0.0 : w * f.wx[k];
    J[4][k] = l ? 0.0 : w * f.wy[k];
    J[5][k] = l ? 0.0 : w * f.wz[k];
  }
  double u[6][6], l[6][6], D[6];  // u holds A, then the factor's u_ij (lower triangle)
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = 0; j <= i; ++j) {
      const int k0 = i == 2 || j == 2;
      double acc = J[i][k0] * J[j][k0];
#pragma unroll
      for (int k = k0 + 1; k < NJ; ++k) acc = acc + J[i][k] * J[j][k];
      u[i][j] = i == j ? acc + lam2 : acc;
    }
#pragma unroll
  for (int j = 0; j < 6; ++j) {
#pragma unroll
    for (int i = j; i < 6; ++i)
#pragma unroll
      for (int k = 0; k < j; ++k) u[i][j] = u[i][j] - l[i][k] * u[j][k];
    D[j] = u[j][j];
#pragma unroll
    for (int i = j + 1; i < 6; ++i) l[i][j] = u[i][j] / D[j];
  }
  double y[6], q[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    y[i] = e[i];
#pragma unroll
    for (int k = 0; k < i; ++k) y[i] = y[i] - l[i][k] * y[k];
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {
    q[i] = y[i] / D[i];
#pragma unroll
    for (int k = i + 1; k < 6; ++k) q[i] = q[i] - l[k][i] * q[k];
  }
#pragma unroll
  for (int k = 0; k < NJ; ++k) {
    double acc = J[0][k] * q[0] + J[1][k] * q[1];
    if (k > 0) acc = acc + J[2][k] * q[2];
#pragma unroll
    for (int r = 3; r < 6; ++r) acc = acc + J[r][k] * q[r];
    d[k] = acc;
  }
}

// chain_step with pose_solve: one step's delta under the limits of P at the angles t;
// returns the lock mask the delta was solved with.
template <int NJ>
IK_ROW_FN unsigned pose_step(const PoseJacN<NJ> &f, const double *e, double w, double lam2,
                             const double *t, const ChainParams &P, double *d, int *resolves) {
  unsigned lock = 0;
  int rs = 0;
  for (;;) {
    pose_solve<NJ>(f, e, w, lam2, lock, d);
    const unsigned nw = chain_new_locks<NJ>(t, d, P, lock);
    lock |= nw;
    rs += nw != 0;
    if (!IK_CHAIN_ANY(nw != 0)) break;
  }
  if (resolves) *resolves = rs;
  return lock;
}

}  // namespace ikhip
