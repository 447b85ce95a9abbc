// ik_fabrik_plan.h -- the host arithmetic of a FABRIK launch (ik_fabrik.hip): the
// loop's threshold, the lazy errors' band, the quotients' domain bound and every
// decision launch_fabrik_ikine takes before it launches.  Plain C++, no HIP header,
// no environment and no state: the code is tested on the CPU
// (tests/test_fabrik_plan_cpu.py).
#pragma once

#include <cstdint>

namespace ikhip {

// The lazy errors' band of one launch (derivation: ik_fabrik_step.h).
struct ErrBand {
  double lo, hi;
};

bool links_core_ok(const double *L, int n);
double tol_threshold(double tol);
ErrBand fabrik_band(double tol2, double n1max, double sum_l);
double fabrik_qmax(const double *L);

struct FabPlanIn {
  double dh[16], links[4];  // RobotDev's
  int64_t n;                // > 0
  double tol;
  int max_iter;
  int variant, core_req, bpc_req;  // the context's IKHIP_FABRIK_VARIANT / _CORE / _BPC
  bool has_table;                  // a cost table was passed
  int order_env, chunk_env;        // IKHIP_FABRIK_ORDER, IKHIP_FABRIK_CHUNK
  int cus;                         // num_cus()
  int ord_ppt, iter_waves;         // IKHIP_ORD_PPT, IKHIP_ITER_WAVES
};

struct FabPlan {
  double tol2;  // tol_threshold(tol)
  ErrBand band;
  double band_n1, qmax;
  bool simple;          // fabrik_simple_kernel alone; nothing below is decided then
  bool ordered = false;  // classify + scatter before the iteration kernel, fold after it
  int core = 0;          // the iteration kernel's CORE
  bool refill1 = false;  // its REFILL_MIN is 1 (variant 2), else IKHIP_FAB_REFILL
  int chunk = 64;
  unsigned grid;  // 256-thread blocks over n (the simple kernel's)
  unsigned ogrid = 0, pgrid = 0;  // classify / scatter blocks; the persistent grid
};

FabPlan fabrik_plan(const FabPlanIn &in);

}  // namespace ikhip
