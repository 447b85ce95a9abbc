// ik_fk_chain.h -- the device FK chain and the per-robot constants
// (RobotConstDev, filled by robot_const_kernel in ik_fk.hip) that the FABRIK seed
// pose, the refine, the analytic solve and the FK round trips read.
#pragma once

#include <hip/hip_runtime.h>

#include "ik_arith.h"
#include "ik_types.h"

namespace ikhip {

// ---------------------------------------------------------------- FK ----
// kinematics/forward.py:21-94.  A_i = Rz(theta)*Tz(d)*Tx(a)*Rx(alpha) and the
// chain M_{i+1} = M_i * A_{i+1}, each 4x4 product an FMA chain in k order from
// 0 (what numpy's dgemm does; pinned bit-exact by the oracle tests).
__device__ __forceinline__ void mm4(const double *A, const double *B, double *C) {
  double T[16];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      double acc = 0.0;
#pragma unroll
      for (int k = 0; k < 4; ++k) acc = fma(A[i * 4 + k], B[k * 4 + j], acc);
      T[i * 4 + j] = acc;
    }
#pragma unroll
  for (int i = 0; i < 16; ++i) C[i] = T[i];
}

__device__ __forceinline__ void ident4(double *M) {
#pragma unroll
  for (int i = 0; i < 16; ++i) M[i] = (i % 5 == 0) ? 1.0 : 0.0;
}

// sin and cos of |x| <= 2 pi (the reference's FK angle range, forward.py:23-25):
// Cody-Waite reduction by pi/2 in three parts, then fdlibm's __kernel_sin /
// __kernel_cos polynomials on [-pi/4, pi/4].  Absolute error <= 1.2e-16 against
// glibc over [-2 pi, 2 pi] (1 ulp for |result| >= 0.5; 2e7 samples, gcc restatement);
// ~40 instructions against ocml's general sincos.  Outside the range the result is
// finite garbage (the FK kernel reports those points as out of range).
__device__ __forceinline__ void sincos_fk(double x, double *sp, double *cp) {
  const double k = __builtin_rint(x * 0.63661977236758134308);
  double r = __builtin_fma(-k, 1.57079632673412561417e+00, x);
  r = __builtin_fma(-k, 6.07710050650619224932e-11, r);
  r = r + (-k * 2.02226624879595063154e-21);
  const double z = r * r;
  const double ps = __builtin_fma(z, __builtin_fma(z, __builtin_fma(z, __builtin_fma(z,
                    __builtin_fma(z, 1.58969099521155010221e-10, -2.50507602534068634195e-08),
                    2.75573137070700676789e-06), -1.98412698298579493134e-04),
                    8.33333333332248946124e-03), -1.66666666666666324348e-01);
  const double sn = __builtin_fma(r * z, ps, r);
  const double pc = __builtin_fma(z, __builtin_fma(z, __builtin_fma(z, __builtin_fma(z,
                    __builtin_fma(z, -1.13596475577881948265e-11, 2.08757232129817482790e-09),
                    -2.75573143513906633035e-07), 2.48015872894767294178e-05),
                    -1.38888888888741095749e-03), 4.16666666666666019037e-02);
  const double hz = 0.5 * z, w = 1.0 - hz;
  const double cs = w + (((1.0 - w) - hz) + z * z * pc);
  const int q = (int)k;
  const double ss = (q & 1) ? cs : sn, cc = (q & 1) ? sn : cs;
  *sp = (q & 2) ? -ss : ss;
  *cp = ((q + 1) & 2) ? -cc : cc;
}

__device__ __forceinline__ bool angle_ok(double a) { return !((a < -2 * kPi) || (a > 2 * kPi)); }

__device__ __forceinline__ void dh_transform(double th, double eps, double a, double al,
                                             double *A) {
  double R[16], T1[16], T2[16], X[16];
  double c = cos(th), s = sin(th);
  ident4(R);
  R[0] = c; R[1] = -s; R[4] = s; R[5] = c;
  ident4(T1);
  T1[11] = eps;
  ident4(T2);
  T2[3] = a;
  double ca = cos(al), sa = sin(al);
  ident4(X);
  X[5] = ca; X[6] = -sa; X[9] = sa; X[10] = ca;
  mm4(R, T1, A);
  mm4(A, T2, A);
  mm4(A, X, A);
}

// dh: rows thetas(unused here), d, a, alpha; th: the 4 joint angles.
// Writes the translations of M_1..M_4.  Returns IK_OK or IK_E_ANGLE_RANGE.
__device__ __forceinline__ int fk_chain(const double *dh, const double th[4], d3 J[4]) {
  int st = IK_OK;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (!angle_ok(th[i]) || !angle_ok(dh[12 + i])) st = IK_E_ANGLE_RANGE;
  double M[16], A[16];
  dh_transform(th[0], dh[4], dh[8], dh[12], M);
  J[0].x = M[3]; J[0].y = M[7]; J[0].z = M[11];
#pragma unroll
  for (int i = 1; i < 4; ++i) {
    dh_transform(th[i], dh[4 + i], dh[8 + i], dh[12 + i], A);
    mm4(M, A, M);
    J[i].x = M[3]; J[i].y = M[7]; J[i].z = M[11];
  }
  return st;
}

// The per-robot constants of the FABRIK seed pose and of the FK round trip
// (RobotConstDev), computed once per robot by robot_const_kernel.
struct RobotConstDev {
  double lim[6];    // workspace limits (inverse.py:26-35)
  double jc[16];    // fk_error's per-joint constants (fk_trip_consts)
  double P[4][3];   // the seed chain's joints at theta_1 = 0 (seed_closed)
  int alpha_bad;
  int st;           // fk_chain's angle check of the constant angles
};
// The robot constants through the constant address space: wave-uniform
// s_load_dwordx* into SGPRs instead of vector loads per lane.
typedef const RobotConstDev __attribute__((address_space(4))) *RcConst;

// The seed pose in closed form.  theta_1 enters the DH chain only through the
// leftmost factor, A_1 = Rz(theta_1) C_1 (forward.py:63-70), so every seed joint
// is J_k = Rz(theta_1) P_k with P_k the chain's joint k at theta_1 = 0 (a robot
// constant), and cos / sin(atan2(y, x)) = (x, y) / |(x, y)|: one reciprocal root
// and four products per joint instead of atan2, cos, sin and three 3 x 4 matrix
// products (r05: ~530 VALU per prepared batch entry).  The joints differ from the
// reference's chain in the last bits of their x / y (for SixDOFRobot those are
// ~1e-16 in size, P_k = (~1e-16, ~1e-16, 2k + 2)): no FABRIK iteration count
// changed over 24M goals at tol 1e-3 .. 1e-8, random_dist and uniform box
// (tools/seed_form_check.c against the oracle's chain).  Goals on the z axis or
// with x^2 + y^2 outside the normal range (and NaN) take cos / sin of atan2 itself
// in a wave-uniform branch.  Returns the robot's constant status.
__device__ __forceinline__ int seed_closed(const RobotConstDev *rc, d3 g, d3 J[4]) {
  const RcConst k = (RcConst)rc;
  const double t = g.x * g.x + g.y * g.y;
  const bool fast = t >= 0x1p-1000 && t <= 0x1p1000;
  // 1 / sqrt(t): the hardware estimate and two coupled Newton steps (sqrt_core's
  // g / h iteration: h -> 1 / (2 sqrt(t)) within a few ulps)
  const double y0 = __builtin_amdgcn_rsq(t);
  double h = 0.5 * y0, gg = t * y0;
  double e = __builtin_fma(-h, gg, 0.5);
  h = __builtin_fma(h, e, h);
  gg = __builtin_fma(gg, e, gg);
  e = __builtin_fma(-h, gg, 0.5);
  h = __builtin_fma(h, e, h);
  double c = g.x * (2.0 * h), s = g.y * (2.0 * h);
  if (__builtin_expect(__any(!fast), 0)) {
    if (!fast) {
      const double th = atan2(g.y, g.x);
      c = cos(th);
      s = sin(th);
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const double px = k->P[j][0], py = k->P[j][1];
    J[j].x = __builtin_fma(c, px, -(s * py));
    J[j].y = __builtin_fma(s, px, c * py);
    J[j].z = k->P[j][2];
  }
  return k->st;
}

// The FK round trip of one point (cli.py:54-61 + the distance to the target),
// register-lean: the effector is Rz(t1) B1 Rz(t2) B2 Rz(t3) B3 Rz(t4) B4 e4
// with B_i = Tz(d_i) Tx(a_i) Rx(alpha_i) (forward.py:63-70 regrouped),
// applied right to left to a vector; jc[i] = {a_i, d_i, cos alpha_i, sin alpha_i}
// from the host (fk_trip_consts).  Same value as fk_chain up to rounding (~1e-15).
// The chain of fk_error from the angles' cosines and sines (c[i], s[i]) and
// whether every angle passed forward.py:23-25's range check (ok).
__device__ __forceinline__ double fk_error_cs(const double *jc, const double c[4],
                                              const double s[4], bool ok, double px, double py,
                                              double pz) {
  double x = jc[12], y = 0.0, z = jc[13];  // B4 e4 = (a4, 0, d4)
#pragma unroll
  for (int i = 3; i >= 0; --i) {
    double xr = c[i] * x - s[i] * y, yr = s[i] * x + c[i] * y;  // Rz(t_i)
    x = xr;
    y = yr;
    if (i > 0) {  // B_{i} (1-based), i.e. jc[i - 1]
      const double *b = jc + 4 * (i - 1);
      double yb = b[2] * y - b[3] * z, zb = b[3] * y + b[2] * z + b[1];
      x = x + b[0];
      y = yb;
      z = zb;
    }
  }
  d3 e = {x, y, z}, p = {px, py, pz};
  return ok ? dist3(e, p) : __builtin_nan("");
}

__device__ __forceinline__ double fk_error(const double *jc, const double th[4], double px,
                                           double py, double pz, int alpha_bad) {
  bool ok = !alpha_bad;
  double c[4], s[4];
#pragma unroll
  for (int i = 3; i >= 0; --i) {
    ok = ok && angle_ok(th[i]);
    sincos_fk(th[i], &s[i], &c[i]);  // |th| <= 2 pi here (ok); outside, the result is NaN anyway
  }
  return fk_error_cs(jc, c, s, ok, px, py, pz);
}

// Same chain, writing all four cumulative transforms (row-major 4x4 each).
__device__ __forceinline__ int fk_chain_mats(const double *dh, const double th[4], double *out) {
  int st = IK_OK;
  for (int i = 0; i < 4; ++i)
    if (!angle_ok(th[i]) || !angle_ok(dh[12 + i])) st = IK_E_ANGLE_RANGE;
  double M[16], A[16];
  dh_transform(th[0], dh[4], dh[8], dh[12], M);
  for (int k = 0; k < 16; ++k) out[k] = M[k];
  for (int i = 1; i < 4; ++i) {
    dh_transform(th[i], dh[4 + i], dh[8 + i], dh[12 + i], A);
    mm4(M, A, M);
    for (int k = 0; k < 16; ++k) out[16 * i + k] = M[k];
  }
  return st;
}

}  // namespace ikhip
