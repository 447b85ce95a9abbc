// ik_fabrik_angles.h -- the angles step of a FABRIK solve (device only): the
// reference's __get_angles in the general arithmetic and through the cheaper core
// sequences with fitted acos / atan2.  Used by ik_fabrik.hip's angles_step.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ik_arith.h"
#include "ik_types.h"

namespace ikhip {

// kinematics/inverse.py:54-112 __get_angles; J = FABRIK joints B, C, D, E.
__device__ __forceinline__ void get_angles(const d3 J[4], double th[4], int &st) {
  const d3 A = {0.0, 0.0, 0.0};
  const d3 B = J[0], C = J[1], D = J[2], E = J[3];
  th[0] = atan2(E.y, E.x);
  double ab = dist3(A, B), bc = dist3(B, C), cd = dist3(C, D), de = dist3(D, E);
  double ac = dist3(A, C);
  double num = (sq(ab) + sq(bc)) - sq(ac);
  double den = 2 * ab * bc;
  double a2 = py_acos(py_round8(py_div(num, den, st)), st);
  th[1] = (C.x * D.x < 0) ? ((3 * kPi / 2) - a2) : -(kPi / 2 - a2);
  double bd = dist3(B, D);
  num = (sq(bc) + sq(cd)) - sq(bd);
  den = 2 * bc * cd;
  double a3 = py_acos(py_round8(py_div(num, den, st)), st);
  th[2] = -(kPi - a3);
  double ce = dist3(C, E);
  num = (sq(cd) + sq(de)) - sq(ce);
  den = 2 * cd * de;
  double a4 = py_acos(py_round8(py_div(num, den, st)), st);
  d3 m = point_between(C, E, dist3(C, E) / 2, st);
  double da = dist3(B, m);
  double db = dist3(B, D);
  th[3] = (db > da) ? -(kPi - a4) : (kPi - a4);
}

// ---- the angles step through cheaper sequences ------------
// Everything __get_angles compares or rounds -- the distances, the law-of-
// cosines quotients, round(., 8), the C.x D.x and |B - D| > |B - m| tests -- must
// keep the reference's bits (a different round(., 8) moves an angle by up to
// 1e-4 near a straight joint).  sqrt_core / div_core give those bits on their
// domains (ik_arith.h).  Only the final math.acos / math.atan2 values leave
// the kernel, and those need not be glibc's last bit (ocml's never were): the
// angles are held to 1e-9 of the oracle (the north star's tolerance is 1e-5).
// acos_fast / atan2_fast: polynomials fitted against mpmath (asin on [0, 1/2],
// degree 11 in u^2, <= 2.1 ulp; atan on [0, tan(pi/8)], degree 10, <= 1 ulp), the
// usual reductions, pi split in two parts.  ~40 VALU instructions each against
// ~100 (ocml acos) and ~114 (ocml atan2).
constexpr double kPio2Hi = 0x1.921fb54442d18p0, kPio2Lo = 0x1.1a62633145c07p-54;
constexpr double kPio4Hi = 0x1.921fb54442d18p-1, kPio4Lo = 0x1.1a62633145c07p-55;
constexpr double kPiHi = 0x1.921fb54442d18p1, kPiLo = 0x1.1a62633145c07p-53;

// asin(u) for u in [0, 1/2]: u + u z P(z), z = u^2 (z passed in)
__device__ __forceinline__ double asin_small(double u, double z) {
  double p = 0x1.c4e4e17088d7fp-6;
  p = __builtin_fma(p, z, -0x1.478579af5a664p-7);
  p = __builtin_fma(p, z, 0x1.fe14951c32a4cp-7);
  p = __builtin_fma(p, z, 0x1.0524bf7ebc431p-7);
  p = __builtin_fma(p, z, 0x1.83eb350c10662p-7);
  p = __builtin_fma(p, z, 0x1.c89fb23c062d2p-7);
  p = __builtin_fma(p, z, 0x1.1c5717f04e8d6p-6);
  p = __builtin_fma(p, z, 0x1.6e8b4bd3059d9p-6);
  p = __builtin_fma(p, z, 0x1.f1c71e76e5bd8p-6);
  p = __builtin_fma(p, z, 0x1.6db6db6aaeb82p-5);
  p = __builtin_fma(p, z, 0x1.3333333335124p-4);
  p = __builtin_fma(p, z, 0x1.555555555555fp-3);
  return __builtin_fma(u * z, p, u);
}

// atan(t) for |t| <= tan(pi/8): t + t s P(s), s = t^2
__device__ __forceinline__ double atan_small(double t) {
  const double s = t * t;
  double p = -0x1.f318cc05bca37p-7;
  p = __builtin_fma(p, s, 0x1.2487560b8b924p-5);
  p = __builtin_fma(p, s, -0x1.959b5ed0b32b2p-5);
  p = __builtin_fma(p, s, 0x1.dd91ab8788317p-5);
  p = __builtin_fma(p, s, -0x1.10d3fc8f710cbp-4);
  p = __builtin_fma(p, s, 0x1.3b0f4916f8726p-4);
  p = __builtin_fma(p, s, -0x1.745ce3b26915fp-4);
  p = __builtin_fma(p, s, 0x1.c71c705fa87fap-4);
  p = __builtin_fma(p, s, -0x1.24924921fc848p-3);
  p = __builtin_fma(p, s, 0x1.99999999958a3p-3);
  p = __builtin_fma(p, s, -0x1.5555555555541p-2);
  return __builtin_fma(t * s, p, t);
}

// math.acos on [-1, 1] (NaN outside, and for NaN): |x| <= 1/2 as pi/2 -+ asin|x|,
// else 2 asin(sqrt((1 - |x|) / 2)) (x > 0) or pi minus it; 1 - |x| is exact there.
__device__ __forceinline__ double acos_fast(double x) {
  const double ax = fabs(x);
  const bool small = ax <= 0.5;
  const double zl = (1.0 - ax) * 0.5;  // 0 or >= 2^-54: sqrt_core's domain or 0
  const double z = small ? x * x : zl;
  const double u = small ? ax : (zl > 0.0 ? sqrt_core(zl) : 0.0);
  const double p = asin_small(u, z);
  const double r_small = x >= 0.0 ? kPio2Hi - (p - kPio2Lo) : kPio2Hi + (p + kPio2Lo);
  const double r_large = x > 0.0 ? 2.0 * p : kPiHi - (2.0 * p - kPiLo);
  const double r = small ? r_small : r_large;
  return ax <= 1.0 ? r : __builtin_nan("");
}

// math.atan2 where both |x| and |y| are in [2^-100, 2^100] (div_core's domain);
// the caller sends zeros, non-finite and extreme values to the library's atan2.
__device__ __forceinline__ double atan2_fast(double y, double x) {
  const double ax = fabs(x), ay = fabs(y);
  const bool swap = ay > ax;
  const double r = div_core(swap ? ax : ay, swap ? ay : ax);  // [0, 1]
  const bool red = r > 0x1.a827999fcef32p-2;  // tan(pi/8): atan r = pi/4 + atan((r-1)/(r+1))
  const double t = red ? div_core(r - 1.0, r + 1.0) : r;
  double a = atan_small(t);
  a = red ? kPio4Hi + (a + kPio4Lo) : a;
  a = swap ? kPio2Hi - (a - kPio2Lo) : a;
  a = x < 0.0 ? kPiHi - (a - kPiLo) : a;
  return copysign(a, y);
}

__device__ __forceinline__ bool in_div_domain(double v) {
  const double a = fabs(v);
  return a >= 0x1p-100 && a <= 0x1p100;
}

// dist3 through sqrt_core (same bits where dom stays below kCoreDom)
__device__ __forceinline__ double dist3c(d3 a, d3 b, uint32_t &dom) {
  const double x = dist3_sq(a, b);
  dom = max(dom, sqrt_core_dom(x));
  return sqrt_core(x);
}

// round(v, 8) (py_round8) with the final k / 1e8 through div_core
__device__ __forceinline__ double py_round8_core(double v, bool &ok) {
  const double s = 1e8;
  const double p = v * s;
  if (!isfinite(p)) return v;
  const double e = fma(v, s, -p);
  const double fl = floor(p);
  double k;
  if (p - fl == 0.5) {
    k = (e > 0) ? fl + 1.0 : ((e < 0) ? fl : rint(p));
  } else {
    k = rint(p);
  }
  ok = ok && (k == 0.0 || in_div_domain(k));
  double r = div_core(k, s);
  if (r == 0.0) r = copysign(0.0, v);
  return r;
}

// sqrt(1 - v^2) = sin(acos(v)) for |v| <= 1 (the FK round trip's sines): 1 - v^2
// in one rounding (fma), its root from the hardware estimate and one coupled
// Newton step -- a few ulps, far inside the round trip's 1e-12 (its value is only
// reported, never compared: tests/test_gpu_parity.py
// ::test_fabrik_fk_err_equals_standalone_fk).
__device__ __forceinline__ double sin_of_acos(double v) {
  const double t = __builtin_fma(-v, v, 1.0);
  const double y = __builtin_amdgcn_rsq(t);
  const double h = 0.5 * y, g = t * y;
  const double e = __builtin_fma(-h, g, 0.5);
  return t > 0.0 ? __builtin_fma(g, e, g) : 0.0;
}

// __get_angles (inverse.py:54-112) through the core sequences; returns false
// (and the caller runs get_angles) when some radicand or quotient leaves their
// domains -- coincident joints, a zero divisor, non-finite joints -- or the
// effector's x or y is zero or extreme (atan2's special cases).
// cs / sn: the angles' cosines and sines for the FK round trip (cli.py:54-61),
// from the values the angles come from instead of sin / cos of the angles:
// theta_1 = atan2(E.y, E.x) gives (E.x, E.y) / |(E.x, E.y)|, and every other angle
// is +-(k pi / 2 -+ acos(v)) of a law-of-cosines value v, so its cosine and sine
// are +-v and +-sqrt(1 - v^2).  They differ from sin / cos of the rounded angles
// by a few ulps (the rounding of the angles themselves), not 4 x 40 instructions.
__device__ __forceinline__ bool get_angles_core(const d3 J[4], double th[4], int &st,
                                                double cs[4], double sn[4]) {
  const d3 A = {0.0, 0.0, 0.0};
  const d3 B = J[0], C = J[1], D = J[2], E = J[3];
  uint32_t dom = 0;
  bool ok = in_div_domain(E.x) && in_div_domain(E.y);
  const double ab = dist3c(A, B, dom), bc = dist3c(B, C, dom), cd = dist3c(C, D, dom),
               de = dist3c(D, E, dom);
  const double ac = dist3c(A, C, dom);
  auto quot = [&](double num, double den) {
    ok = ok && (num == 0.0 || in_div_domain(num)) && in_div_domain(den);
    return div_core(num, den);
  };
  auto acos_py = [&](double v) {
    if (v > 1.0 || v < -1.0) set_err(st, IK_E_DOMAIN);
    return acos_fast(v);
  };
  double num = (sq(ab) + sq(bc)) - sq(ac);
  double den = 2 * ab * bc;
  const double v2 = py_round8_core(quot(num, den), ok);
  const double a2 = acos_py(v2);
  const bool up = C.x * D.x < 0;
  th[1] = up ? ((3 * kPi / 2) - a2) : -(kPi / 2 - a2);
  const double w2 = sin_of_acos(v2);
  cs[1] = up ? -w2 : w2;  // cos(3 pi / 2 - a) = -sin a, cos(a - pi / 2) = sin a
  sn[1] = -v2;            // sin of either is -cos a
  const double bd = dist3c(B, D, dom);
  num = (sq(bc) + sq(cd)) - sq(bd);
  den = 2 * bc * cd;
  const double v3 = py_round8_core(quot(num, den), ok);
  const double a3 = acos_py(v3);
  th[2] = -(kPi - a3);
  cs[2] = -v3;  // a - pi
  sn[2] = -sin_of_acos(v3);
  const double ce = dist3c(C, E, dom);
  num = (sq(cd) + sq(de)) - sq(ce);
  den = 2 * cd * de;
  const double v4 = py_round8_core(quot(num, den), ok);
  const double a4 = acos_py(v4);
  // get_point_between(C, E, |C - E| / 2): |C - E| is ce again (the radicand squares
  // E - C = -(C - E) exactly) and (ce / 2) / ce is exactly 0.5 for a ce in the domain
  const d3 m = {C.x + (0.5 * (E.x - C.x)), C.y + (0.5 * (E.y - C.y)), C.z + (0.5 * (E.z - C.z))};
  const double da = dist3c(B, m, dom);
  th[3] = (bd > da) ? -(kPi - a4) : (kPi - a4);  // db = |B - D| = bd
  cs[3] = -v4;  // a - pi or pi - a
  const double w4 = sin_of_acos(v4);
  sn[3] = (bd > da) ? -w4 : w4;
  // th[0] = atan2_fast(E.y, E.x): by the caller, after the fallback pass; its
  // cosine and sine from E (E.x, E.y in the division domain: t is normal)
  {
    const double t = E.x * E.x + E.y * E.y;
    const double y = __builtin_amdgcn_rsq(t);
    const double h = 0.5 * y, g = t * y;
    const double e = __builtin_fma(-h, g, 0.5);
    const double yi = __builtin_fma(y, e, y);
    cs[0] = E.x * yi;
    sn[0] = E.y * yi;
  }
  return ok && dom < kCoreDom;
}

}  // namespace ikhip
