// ik_arith.h -- device arithmetic that restates Python's, shared by the FK /
// FABRIK / ANN kernels.
//
// Float64 arithmetic here follows the reference's operation order exactly and
// the whole library is compiled with -ffp-contract=off (CPython never fuses a
// multiply-add), so that FABRIK iteration counts match the reference bit for
// bit.  The one deliberate difference: the reference squares with pow(v, 2)
// (glibc pow, kinematics/point.py:27-29, inverse.py:79,90,98), here v*v, the
// correctly rounded square; glibc pow differs from it in the last ulp on a
// small fraction of inputs.  See DESIGN.md "Numerics".
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "ik_types.h"

namespace ikhip {

// The reference's pow(v, 2).
__device__ __forceinline__ double sq(double v) { return v * v; }

// kinematics/point.py:25-29 get_distance_between, and its radicand
__device__ __forceinline__ double dist3_sq(d3 a, d3 b) {
  return sq(a.x - b.x) + sq(a.y - b.y) + sq(a.z - b.z);
}
__device__ __forceinline__ double dist3(d3 a, d3 b) { return sqrt(dist3_sq(a, b)); }

__device__ __forceinline__ void set_err(int &st, int code) {
  if (st == IK_OK) st = code;
}

// kinematics/point.py:32-45 get_point_between: s_c + ((d / |s-e|) * (e_c - s_c)).
// |s-e| == 0 raises ZeroDivisionError in the reference.  The differences are
// formed once: the distance squares s_c - e_c and fl(s_c - e_c) = -fl(e_c - s_c)
// exactly, so squaring e_c - s_c gives the same radicand bit for bit.
__device__ __forceinline__ d3 point_between(d3 s, d3 e, double d, int &st) {
  const double dx = e.x - s.x, dy = e.y - s.y, dz = e.z - s.z;
  double n = sqrt(sq(dx) + sq(dy) + sq(dz));
  if (n == 0.0) set_err(st, IK_E_ZERODIV);
  double q = d / n;
  d3 r;
  r.x = s.x + (q * dx);
  r.y = s.y + (q * dy);
  r.z = s.z + (q * dz);
  return r;
}

// The compiler's correctly rounded float64 sqrt and division (the AMDGPU
// lowerings of llvm.sqrt.f64 and fdiv double) are a Newton sequence wrapped in
// range handling: sqrt scales radicands below 2^-767 by 2^256 and patches 0/inf
// with v_cmp_class + selects; division pre/post-scales with v_div_scale /
// v_div_fmas and patches specials with v_div_fixup.  Where none of that fires
// the result is the bare sequence below, instruction for instruction, so these
// give the same bits as sqrt() / operator/ on their domains:
//   sqrt_core(x): 2^-767 <= x < 2^1024 (the high word of x in [hi(2^-767),
//     hi(+inf)), which also rejects 0, negatives and NaN);
//   div_core(a, b): b = sqrt_core(x) for such an x and 2^-100 <= |a| <= 2^100
//   (no v_div_scale case: exponent gap < 768, quotient and 1/b normal, a not tiny).
__device__ __forceinline__ double sqrt_core(double x) {
  const double y = __builtin_amdgcn_rsq(x);
  double g = x * y;
  double h = y * 0.5;
  const double r = __builtin_fma(-h, g, 0.5);
  g = __builtin_fma(g, r, g);
  h = __builtin_fma(h, r, h);
  double e = __builtin_fma(-g, g, x);
  g = __builtin_fma(e, h, g);
  e = __builtin_fma(-g, g, x);
  return __builtin_fma(e, h, g);
}
__device__ __forceinline__ double div_core(double a, double b) {
  double r = __builtin_amdgcn_rcp(b);
  double e = __builtin_fma(-b, r, 1.0);
  r = __builtin_fma(r, e, r);
  e = __builtin_fma(-b, r, 1.0);
  r = __builtin_fma(r, e, r);
  const double q = a * r;
  const double res = __builtin_fma(-b, q, a);
  return __builtin_fma(res, r, q);
}

// point_between through sqrt_core / div_core.  dom accumulates the radicands'
// distance from sqrt_core's domain (sqrt_core_dom: max over calls < kCoreDom
// <=> all in the domain); d must be in div_core's (checked once on the host).
// Where the domain holds the result equals point_between's and no error is
// possible.
constexpr uint32_t kCoreDom = 0x6FF00000u;
__device__ __forceinline__ uint32_t sqrt_core_dom(double x) {
  return (uint32_t)__double2hiint(x) - 0x10000000u;
}
__device__ __forceinline__ d3 point_between_core(d3 s, d3 e, double d, uint32_t &dom) {
  const double dx = e.x - s.x, dy = e.y - s.y, dz = e.z - s.z;
  const double x = sq(dx) + sq(dy) + sq(dz);
  dom = max(dom, sqrt_core_dom(x));
  const double q = div_core(d, sqrt_core(x));
  d3 r;
  r.x = s.x + (q * dx);
  r.y = s.y + (q * dy);
  r.z = s.z + (q * dz);
  return r;
}

// CPython round(v, 8): exact value of v rounded half-even to 8 decimals, then
// the nearest double.  v*1e8 = p + e exactly; e breaks a tie at p = k + 1/2.
__device__ __forceinline__ double py_round8(double v) {
  const double s = 1e8;
  double p = v * s;
  if (!isfinite(p)) return v;
  double e = fma(v, s, -p);
  double fl = floor(p);
  double k;
  if (p - fl == 0.5) {
    k = (e > 0) ? fl + 1.0 : ((e < 0) ? fl : rint(p));
  } else {
    k = rint(p);
  }
  double r = k / s;
  if (r == 0.0) r = copysign(0.0, v);
  return r;
}

// math.acos: ValueError('math domain error') outside [-1, 1]; nan passes.
__device__ __forceinline__ double py_acos(double v, int &st) {
  if (v > 1.0 || v < -1.0) set_err(st, IK_E_DOMAIN);
  return acos(v);
}

// float division: ZeroDivisionError when the divisor is zero.
__device__ __forceinline__ double py_div(double a, double b, int &st) {
  if (b == 0.0) set_err(st, IK_E_ZERODIV);
  return a / b;
}

}  // namespace ikhip
