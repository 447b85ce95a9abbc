// ik_chain_row.h -- one row of ik_chain_solve (include/ikhip.h "Chain solve"): the
// forward-kinematics chain of NJ revolute joints with its Jacobian, the damped
// least-squares solve with a lock mask, the active-set step under joint limits, the
// 0.5 rad scaling, the placing of a start point and the start-point hash of the
// restarts.  It is ik_chain_jac.h and ik_refine_step.h with NJ where those say 4: at
// NJ = 4 every value is computed by the same IEEE operations in the same order, so
// the bits are ik_refine's.  Compiled by the kernel (ik_chain.hip) and by a plain host
// compiler (tests/host/chain_row_check.cpp), -ffp-contract=off in both;
// kinematics/chain.py restates it in numpy.  Needs no HIP header.
#pragma once

#include <stdint.h>

#include "ik_row.h"

// Whether any lane of the wave holds p (a builtin: this header needs no HIP header); on
// the host, the row's own p.
#if defined(__HIP_DEVICE_COMPILE__)
#define IK_CHAIN_ANY(p) (__builtin_amdgcn_ballot_w64(p) != 0)
#else
#define IK_CHAIN_ANY(p) (p)
#endif

namespace ikhip {

constexpr int kChainMinJoints = 2, kChainMaxJoints = 8;

// What the kernel takes by value (wave-uniform): per joint {a_i, d_i, cos alpha_i,
// sin alpha_i} as fk_trip_consts computes them, the joint limits (bit i of mask:
// joint i is limited, lo[i] <= hi[i] both inside [-pi, pi]; a free joint holds
// -inf / +inf) and whether some |alpha_i| > 2 pi.
struct ChainParams {
  double jc[kChainMaxJoints][4];
  double lo[kChainMaxJoints], hi[kChainMaxJoints];
  unsigned mask;
  int alpha_bad;
};

// The effector and the Jacobian's columns (jz[0] is identically zero and is never
// read).
template <int NJ>
struct ChainJacN {
  double x, y, z;
  double jx[NJ], jy[NJ], jz[NJ];
};

// Rz(t_1) B_1 Rz(t_2) B_2 .. Rz(t_NJ) B_NJ e4, B_i = Tz(d_i) Tx(a_i) Rx(alpha_i),
// applied right to left to a vector, the open columns riding along: column i is
// (-y', x', 0) of the vector just rotated by Rz(t_i), then takes only the rotations
// to its left.  s, c: the sines and cosines of the NJ angles.
template <int NJ>
IK_ROW_FN ChainJacN<NJ> chain_jac(const double (*jc)[4], const double *s, const double *c) {
  ChainJacN<NJ> f;
  double x = jc[NJ - 1][0], y = 0.0, z = jc[NJ - 1][1];  // B_NJ e4 = (a, 0, d)
#pragma unroll
  for (int i = NJ - 1; i >= 0; --i) {
    const double ci = c[i], si = s[i];
    const double xr = ci * x - si * y, yr = si * x + ci * y;  // Rz(t_i)
#pragma unroll
    for (int k = i + 1; k < NJ; ++k) {  // ... on the columns to its right
      const double wx = ci * f.jx[k] - si * f.jy[k], wy = si * f.jx[k] + ci * f.jy[k];
      f.jx[k] = wx;
      f.jy[k] = wy;
    }
    f.jx[i] = -yr;  // d Rz(t_i) v / dt_i
    f.jy[i] = xr;
    f.jz[i] = 0.0;
    x = xr;
    y = yr;
    if (i > 0) {  // B_i (1-based): Rx(alpha), then the translations (a, 0, d)
      const double a = jc[i - 1][0], d = jc[i - 1][1], ca = jc[i - 1][2], sa = jc[i - 1][3];
      const double yb = ca * y - sa * z, zb = sa * y + ca * z + d;
      x = x + a;
      y = yb;
      z = zb;
#pragma unroll
      for (int k = i; k < NJ; ++k) {
        const double wy = ca * f.jy[k] - sa * f.jz[k], wz = sa * f.jy[k] + ca * f.jz[k];
        f.jy[k] = wy;
        f.jz[k] = wz;
      }
    }
  }
  f.x = x;
  f.y = y;
  f.z = z;
  return f;
}

// d[0..NJ-1] = J'^T (J' J'^T + lam2 I)^-1 e, J' = J with the columns in `lock`
// replaced by +0.0 (a select, not a product).  Every entry of A is a sum over the
// joints in joint order, lam2 added last; LDL^T without pivoting.
template <int NJ>
IK_ROW_FN void chain_solve(const ChainJacN<NJ> &f, double ex, double ey, double ez, double lam2,
                           unsigned lock, double *d) {
  double jx[NJ], jy[NJ], jz[NJ];
#pragma unroll
  for (int k = 0; k < NJ; ++k) {
    const bool l = (lock >> k) & 1u;
    jx[k] = l ? 0.0 : f.jx[k];
    jy[k] = l ? 0.0 : f.jy[k];
    jz[k] = l ? 0.0 : f.jz[k];
  }
  double A00 = jx[0] * jx[0], A10 = jy[0] * jx[0], A11 = jy[0] * jy[0];
  double A20 = jz[1] * jx[1], A21 = jz[1] * jy[1], A22 = jz[1] * jz[1];
#pragma unroll
  for (int k = 1; k < NJ; ++k) {
    A00 = A00 + jx[k] * jx[k];
    A10 = A10 + jy[k] * jx[k];
    A11 = A11 + jy[k] * jy[k];
  }
#pragma unroll
  for (int k = 2; k < NJ; ++k) {
    A20 = A20 + jz[k] * jx[k];
    A21 = A21 + jz[k] * jy[k];
    A22 = A22 + jz[k] * jz[k];
  }
  A00 = A00 + lam2;
  A11 = A11 + lam2;
  A22 = A22 + lam2;
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
  d[0] = jx[0] * q0 + jy[0] * q1;
#pragma unroll
  for (int k = 1; k < NJ; ++k) d[k] = jx[k] * q0 + jy[k] * q1 + jz[k] * q2;
}

// The limited joints outside `lock` that sit on a bound with delta pointing out.
template <int NJ>
IK_ROW_FN unsigned chain_new_locks(const double *t, const double *d, const ChainParams &P,
                                   unsigned lock) {
  unsigned nw = 0;
#pragma unroll
  for (int i = 0; i < NJ; ++i) {
    const bool out = ((t[i] <= P.lo[i]) & (d[i] < 0.0)) | ((t[i] >= P.hi[i]) & (d[i] > 0.0));
    nw |= (out ? 1u : 0u) << i;
  }
  return nw & P.mask & ~lock;
}

// One step's delta under the limits of P at the angles t (inside the limits);
// returns the lock mask the delta was solved with.  Locks only grow: at most NJ
// re-solves.  On the device the loop is wave-uniform, as refine_step's.  resolves
// (nullable): solves after the first that changed this row's mask.
template <int NJ>
IK_ROW_FN unsigned chain_step(const ChainJacN<NJ> &f, double ex, double ey, double ez,
                              double lam2, const double *t, const ChainParams &P, double *d,
                              int *resolves) {
  unsigned lock = 0;
  int rs = 0;
  for (;;) {
    chain_solve<NJ>(f, ex, ey, ez, lam2, lock, d);
    const unsigned nw = chain_new_locks<NJ>(t, d, P, lock);
    lock |= nw;
    rs += nw != 0;
    if (!IK_CHAIN_ANY(nw != 0)) break;
  }
  if (resolves) *resolves = rs;
  return lock;
}

// delta scaled so that max |delta_i| <= clamp (0.5 rad).
template <int NJ>
IK_ROW_FN void chain_scale(double *d, double clamp) {
  double m = fabs(d[0]);
#pragma unroll
  for (int k = 1; k < NJ; ++k) m = fmax(m, fabs(d[k]));
  if (m > clamp) {
    const double sc = clamp / m;
#pragma unroll
    for (int k = 0; k < NJ; ++k) d[k] = d[k] * sc;
  }
}

// t pulled into [lo, hi]; a NaN stays NaN (ik_refine_step.h's refine_project).
IK_ROW_FN double chain_clip(double t, double lo, double hi) {
  t = t < lo ? lo : t;
  return t > hi ? hi : t;
}

// What a seed, a restart's start point and an updated angle get: a limited joint
// (kLimited and its mask bit) is pulled into [lo, hi], a free one is wrapped.
template <bool kLimited>
IK_ROW_FN double chain_place(double t, const ChainParams &P, int j) {
  if (kLimited) return ((P.mask >> j) & 1u) ? chain_clip(t, P.lo[j], P.hi[j]) : wrap_pi(t);
  return wrap_pi(t);
}

// The uniform number in [0, 1) of (row, attempt a >= 1, joint j): splitmix64's
// finalizer on row * golden + ((a << 8) | j), its top 53 bits.
IK_ROW_FN double chain_start_u(uint64_t row, unsigned a, unsigned j) {
  uint64_t z = row * 0x9E3779B97F4A7C15ull + (uint64_t)((a << 8) | j);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (double)(z >> 11) * 0x1p-53;
}

// Attempt a's start of joint j, before chain_place: lo' + u (hi' - lo'), [lo', hi']
// the joint's limits, or [-pi, pi] for a free joint.
template <bool kLimited>
IK_ROW_FN double chain_start(uint64_t row, unsigned a, int j, const ChainParams &P) {
  const double pi = 3.141592653589793;
  double lo = -pi, hi = pi;
  if (kLimited) {
    const bool lim = (P.mask >> j) & 1u;
    lo = lim ? P.lo[j] : lo;
    hi = lim ? P.hi[j] : hi;
  }
  return lo + chain_start_u(row, a, (unsigned)j) * (hi - lo);
}

}  // namespace ikhip
