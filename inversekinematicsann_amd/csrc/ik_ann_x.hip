// The split-mode (bf16x6, fp16x3) instantiations of ann_fused_kernel, compiled
// apart from the fp32 kernel: in one module with it they change its register
// allocation (29 -> 51 spilled VGPRs at MR = 2, -Rpass-analysis=kernel-resource-usage).
#include "ik_ann_kernel.h"

namespace ikhip {
using namespace ann;

void ann::launch_ann_kernel_x(int mr, int xmode, unsigned grid, hipStream_t st,
                              const AnnArgs &a) {
#define IK_X(M, X) \
  IK_LAUNCH((ann_fused_kernel<M, X>), dim3(grid), dim3(64 * ann_waves<M, X>()), 0, st, a)
  if (mr == 2) {
    if (xmode == 2) IK_X(2, 2); else IK_X(2, 1);
  } else {
    if (xmode == 2) IK_X(1, 2); else IK_X(1, 1);
  }
#undef IK_X
}

}  // namespace ikhip
