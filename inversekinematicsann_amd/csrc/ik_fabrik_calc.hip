// ik_fabrik_calc.hip -- Fabrik.calculate (kinematics/fabrik.py:19-67) for a chain
// of any length: one goal per lane in float64, the reference's operation order
// (point_between, ik_arith.h), the chain in registers up to 8 joints and in the
// lane's output row past that.
#include "ik_arith.h"
#include "ik_fabrik.h"
#include "ik_fabrik_plan.h"
#include "ik_launch.h"
#include "ik_stats.h"

namespace ikhip {

// ------------------------------------------------------ Fabrik.calculate ----
template <int NJ>
__global__ __launch_bounds__(256) void fabrik_calc_kernel(const double *dists_in,
                                                          const double *init, int shared,
                                                          const double *goals, int64_t n,
                                                          double tol2, int max_iter,
                                                          double *joints, int32_t *iters,
                                                          DevStats *S) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool valid = i < n;
  int it = 0;
  if (valid) {
    double L[NJ];
#pragma unroll
    for (int k = 0; k < NJ; ++k) L[k] = dists_in[k];
    const double *ip = shared ? init : init + (size_t)i * NJ * 3;
    d3 cur[NJ], B[NJ];
#pragma unroll
    for (int k = 0; k < NJ; ++k) cur[k] = {ip[3 * k], ip[3 * k + 1], ip[3 * k + 2]};
    d3 g = {goals[3 * i], goals[3 * i + 1], goals[3 * i + 2]};
    const d3 start = cur[0];
    double se = 1.0, ge = 1.0;
    int st = IK_OK;
    while (((se > tol2) || (ge > tol2)) && (max_iter > it)) {  // squared errors
      B[NJ - 1] = g;
#pragma unroll
      for (int k = NJ - 2; k >= 0; --k) B[k] = point_between(B[k + 1], cur[k], L[k], st);
      se = dist3_sq(B[0], start);
      cur[0] = start;
#pragma unroll
      for (int k = 1; k < NJ; ++k) cur[k] = point_between(cur[k - 1], B[k], L[k], st);
      ge = dist3_sq(cur[NJ - 1], g);
      ++it;
      if (st != IK_OK) break;
    }
    if (st != IK_OK) record_error(S, i, st);
    double *o = joints + (size_t)i * NJ * 3;
#pragma unroll
    for (int k = 0; k < NJ; ++k) {
      o[3 * k] = cur[k].x;
      o[3 * k + 1] = cur[k].y;
      o[3 * k + 2] = cur[k].z;
    }
    if (iters) iters[i] = it;
  }
  block_iter_stats(S, valid, it, max_iter);
}

// Any chain length (1 joint up, fabrik.py:44-67 takes any len(init) ==
// len(dists)): the chain lives in the lane's output row instead of registers.
// The backward pass writes B[k] over cur[k] (cur[k] is read only to form B[k]),
// and the forward pass writes the new cur[k] over B[k] (read only to form it),
// so one nj x 3 row per point holds both passes.  Same point_between calls in the
// same order as the unrolled kernel: the same bits.
__global__ __launch_bounds__(256) void fabrik_calc_any_kernel(int nj, const double *dists,
                                                              const double *init, int shared,
                                                              const double *goals, int64_t n,
                                                              double tol2, int max_iter,
                                                              double *joints, int32_t *iters,
                                                              DevStats *S) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool valid = i < n;
  int it = 0;
  if (valid) {
    const double *ip = shared ? init : init + (size_t)i * nj * 3;
    double *row = joints + (size_t)i * nj * 3;
    auto ld = [&](const double *p, int k) -> d3 { return {p[3 * k], p[3 * k + 1], p[3 * k + 2]}; };
    auto stj = [&](int k, d3 v) {
      row[3 * k] = v.x;
      row[3 * k + 1] = v.y;
      row[3 * k + 2] = v.z;
    };
    for (int k = 0; k < nj; ++k) stj(k, ld(ip, k));
    const d3 g = {goals[3 * i], goals[3 * i + 1], goals[3 * i + 2]};
    const d3 start = ld(ip, 0);
    double se = 1.0, ge = 1.0;
    int st = IK_OK;
    while (((se > tol2) || (ge > tol2)) && (max_iter > it)) {  // squared errors
      d3 b = g;  // B[nj - 1]
      stj(nj - 1, b);
      for (int k = nj - 2; k >= 0; --k) {
        b = point_between(b, ld(row, k), dists[k], st);
        stj(k, b);
      }
      se = dist3_sq(b, start);  // B[0]
      d3 f = start;
      stj(0, f);
      for (int k = 1; k < nj; ++k) {
        f = point_between(f, ld(row, k), dists[k], st);
        stj(k, f);
      }
      ge = dist3_sq(f, g);
      ++it;
      if (st != IK_OK) break;
    }
    if (st != IK_OK) record_error(S, i, st);
    if (iters) iters[i] = it;
  }
  block_iter_stats(S, valid, it, max_iter);
}

void launch_fabrik_calc(int nj, const double *dists, const double *init, bool init_shared,
                        const double *goals, int64_t n, double tol, int max_iter,
                        double *joints, int32_t *iters, DevStats *S, hipStream_t st) {
  if (n <= 0) return;
  unsigned grid = (unsigned)((n + 255) / 256);
  int sh = init_shared ? 1 : 0;
  const double tol2 = tol_threshold(tol);
#define IK_CALC_CASE(K)                                                                      \
  case K:                                                                                    \
    IK_LAUNCH(fabrik_calc_kernel<K>, dim3(grid), dim3(256), 0, st, dists, init, sh, \
                       goals, n, tol2, max_iter, joints, iters, S);                          \
    break;
  kt_begin("fabrik_calc_kernel", st);
  switch (nj) {
    IK_CALC_CASE(2)
    IK_CALC_CASE(3)
    IK_CALC_CASE(4)
    IK_CALC_CASE(5)
    IK_CALC_CASE(6)
    IK_CALC_CASE(7)
    IK_CALC_CASE(8)
    default:
      IK_LAUNCH(fabrik_calc_any_kernel, dim3(grid), dim3(256), 0, st, nj, dists, init,
                         sh, goals, n, tol2, max_iter, joints, iters, S);
      break;
  }
  kt_end(st);
#undef IK_CALC_CASE
}

}  // namespace ikhip
