// The fp32 kernel for models wider than 512 (up to 1024): ik_ann_kernel.h
// compiled with 1028-float LDS rows (IKHIP_ANN_WIDE, namespace annw), 32-point
// tiles (132 KiB of LDS: one workgroup per CU).
#define IKHIP_ANN_WIDE 1
#include "ik_ann_kernel.h"

namespace ikhip {

void launch_ann_wide(const AnnModelDev &m, const RobotDev &r, const double *pts, int64_t n,
                     float *ang, double *fk_err, bool check_limits, DevStats *S, hipStream_t st,
                     unsigned long long *dbg) {
  using namespace annw;
  if (n <= 0) return;
  const AnnArgs a = ann_args(m, r, pts, n, ang, fk_err, check_limits, S, dbg);
  const int64_t ntiles = (n + 31) / 32, cus = num_cus();
  const unsigned grid = (unsigned)(ntiles < cus ? ntiles : cus);
  kt_begin("ann_fused_kernel_wide", st);
  IK_LAUNCH((ann_fused_kernel<1, 0>), dim3(grid), dim3(256), 0, st, a);
  kt_end(st);
}

}  // namespace ikhip
