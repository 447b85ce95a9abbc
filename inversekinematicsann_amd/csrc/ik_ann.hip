// ik_ann.hip -- the fused ANN solve's launcher and its fp32 kernels for widths
// <= 512 (ik_ann_kernel.h; split modes: ik_ann_x.hip, wider models: ik_ann_w.hip).
#include "ik_ann_kernel.h"

namespace ikhip {
using namespace ann;

// Tile rows per workgroup: 32 * MR points.  fp32: MR = 1 (two 32-point
// workgroups per CU, one's barrier and epilogue under the other's MFMAs)
// measured 39.8 ms against 41.3 ms for MR = 2 (1M points, 3-12x500-4,
// tools/sweep_ann.py and bench.py, same box; round 1's GEMM loop measured the
// opposite, 49.0 vs 44.9 ms).  The split modes keep MR = 2: their GEMM is bound
// by the weight stream from L2, which 64-point tiles halve (bf16x6 25.1 vs
// 33.8 ms, fp16x3 15.2 vs 19.6 ms).  IKHIP_ANN_MR overrides.
static int ann_tile_rows(int xmode) {
  static int forced = -1;
  if (forced < 0) {
    const char *v = getenv("IKHIP_ANN_MR");
    forced = (v && (atoi(v) == 1 || atoi(v) == 2)) ? atoi(v) : 0;
  }
  return forced ? forced : (xmode ? 2 : 1);
}

size_t ann_debug_words() { return (size_t)kStampTiles * kWaves * kStampSlots; }

void launch_ann(const AnnModelDev &m, const RobotDev &r, const double *pts, int64_t n,
                float *ang, double *fk_err, bool check_limits, DevStats *S, hipStream_t st,
                unsigned long long *dbg) {
  if (n <= 0) return;
  for (int l = 0; l < m.n_layers; ++l)
    if (m.np[l] > 512 || m.kp[l] > 512) {
      launch_ann_wide(m, r, pts, n, ang, fk_err, check_limits, S, st, dbg);
      return;
    }
  const AnnArgs a = ann_args(m, r, pts, n, ang, fk_err, check_limits, S, dbg);
  bool x = false;
  for (int l = 0; l < m.n_layers; ++l) x = x || m.wx[l] != nullptr;
  const int xmode = x ? m.xmode : 0;
  const int mr = ann_tile_rows(xmode);
  const int64_t bm = 32 * mr;
  const int64_t ntiles = (n + bm - 1) / bm;
  const int64_t slots = (int64_t)num_cus() * (mr == 2 ? 1 : 2);  // resident workgroups
  unsigned grid = (unsigned)(ntiles < slots ? ntiles : slots);
  kt_begin(xmode == 1 ? "ann_fused_kernel_bf16x6"
                      : xmode == 2 ? "ann_fused_kernel_fp16x3" : "ann_fused_kernel",
           st);
  if (xmode)
    launch_ann_kernel_x(mr, xmode, grid, st, a);
  else if (mr == 2)
    IK_LAUNCH((ann_fused_kernel<2, 0>), dim3(grid), dim3(64 * ann_waves<2, 0>()), 0, st, a);
  else
    IK_LAUNCH((ann_fused_kernel<1, 0>), dim3(grid), dim3(256), 0, st, a);
  kt_end(st);
}

}  // namespace ikhip
