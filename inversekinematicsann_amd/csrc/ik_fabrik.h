// ik_fabrik.h -- launchers of the FABRIK units (ik_fabrik.hip: ikine;
// ik_fabrik_calc.hip: Fabrik.calculate) and the work order's cost table, which
// the context owns (ik_fabrik_order.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "ik_launch.h"
#include "ik_types.h"

namespace ikhip {

struct RobotConstDev;  // ik_fk_chain.h

// Fabrik.calculate's chain length bound (ik_fabrik_calc).  Chains past 8 joints
// run one goal per lane with the chain in its output row, so a goal costs about
// nj * max_iter * 2 dependent point_between steps (~0.4 us each, an L2 round
// trip): 4096 joints at 100 iterations is ~0.3 s for a launch of any width
// (tests/test_gpu_parity.py::test_fabrik_calc_longest_chain), well inside the
// GPU's hang detection; longer chains are refused.
constexpr int kCalcMaxJoints = 4096;
// FABRIK work order (ik_fabrik_order.hip "Work order"): per context, the largest
// iteration count recorded in each goal cell (distance x elevation from the
// shoulder) on the context's earlier calls decides which points start first.
constexpr int kOrdCellsR = 64, kOrdCellsE = 16, kOrdCells = kOrdCellsR * kOrdCellsE;
constexpr int kOrdSample = 256;           // 1 point in 256 is recorded ...
constexpr int kOrdMaxSample = 1 << 14;    // ... up to this many per call
struct FabOrderDev {
  unsigned int key[kOrdCells];  // 1 + largest recorded iterations per cell, 0 = unseen
  unsigned int sample[kOrdMaxSample];  // (cell << 16 | iterations) records of the call
};

// FABRIK ikine.  scratch must hold fabrik_scratch_bytes(n).  ord: the
// context's cost table (zero-initialised once), or null for queue order =
// point order.  fk_err (nullable): |FK(theta) - p| per point, max/sum into S.
size_t fabrik_scratch_bytes(int64_t n);
void launch_fabrik_ikine(const RobotDev &r, const double *pts, int64_t n, double tol,
                         int max_iter, double *ang, int32_t *iters, double *joints,
                         double *fk_err, bool check_limits, void *scratch, DevStats *S, hipStream_t st,
                         int variant, int core, FabOrderDev *ord, const RobotConstDev *rc,
                         unsigned long long *dbg, int bpc = 0, bool prior = false);
constexpr size_t kFabrikDebugWords = 64 + 24 * 4096;  // diagnostic build: totals + per-wave records
void launch_fabrik_calc(int nj, const double *dists, const double *init, bool init_shared,
                        const double *goals, int64_t n, double tol, int max_iter,
                        double *joints, int32_t *iters, DevStats *S, hipStream_t st);

}  // namespace ikhip
