// ik_fabrik_args.h -- what the two units of a FABRIK ikine solve share: the
// kernels' argument block (ik_fabrik.hip fills it) and the work-order launches
// around the iteration kernel (ik_fabrik_order.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ik_fabrik.h"
#include "ik_fabrik_plan.h"
#include "ik_launch.h"
#include "ik_types.h"

namespace ikhip {

struct FabArgs {
  RobotDev r;
  const RobotConstDev *rc;  // seed constants (robot_const_kernel)
  const double *pts;
  int64_t n;
  double tol;      // fabrik.py:57 err_margin, as given
  double tol2;     // tol_threshold(tol): the loop compares squared errors with it
  ErrBand band;    // the lazy errors' band (fabrik_band) for lanes with |J0|_1 + |goal|_1 <= band_n1
  double band_n1;
  double qmax;     // the core-domain test on the quotients (fabrik_qmax)
  int max_iter;
  int check_limits;
  double *ang;
  int32_t *iters;   // nullable
  double *joints;   // final joints n x 12 (nullable)
  double *fk_err;   // |FK(theta) - p| per point (nullable; max/sum into S)
  DevStats *S;
  int chunk;        // work-queue grab size of the persistent iteration kernel (1..64)
  // hard-first ordering (ik_fabrik_order.hip "Work order"); unused when perm is null
  int32_t *perm;    // queue position -> point index
  uint16_t *cell;   // per point: goal cell (bits 0-9) | cost class << 10
  FabOrderDev *ord; // context-owned cost table
  int prior_gate;   // the table is a built-in prior no call has taught yet (see scatter)
  unsigned long long *dbg;  // diagnostic build only: iteration-kernel counters
};

// 16 at 1M points: classify + scatter 28.8 us against 34.2 for 8 (table reads early)
// and 49.0 for 4 (same box)
#ifndef IKHIP_ORD_PPT
#define IKHIP_ORD_PPT 16
#endif
constexpr int kOrdPPT = IKHIP_ORD_PPT;  // points per thread of the classify / scatter blocks

// Before the iteration kernel: classify + scatter (a.cell and a.perm from the goals
// and the table), grid blocks of 256 x kOrdPPT points.  After it: the call's
// samples into the table (one block).
void launch_fabrik_order(const FabArgs &a, unsigned grid, hipStream_t st);
void launch_fabrik_fold(const FabArgs &a, hipStream_t st);

}  // namespace ikhip
