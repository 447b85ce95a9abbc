// ik_act.h -- the activation functions, once: the fused inference kernels
// (ik_ann_kernel.h) take the template, the layered path (ik_ann_big.hip) and
// training (ik_train.hip) the run-time form, which dispatches to it -- so a
// trained model predicts what it was trained to, bit for bit.
//
// Hardware exp2 / reciprocal (1 ulp each).  tanh is 1 - 2 / (1 + e),
// e = exp2(2 log2(e) v): one exp, one add, one reciprocal and one fma per element,
// absolute error <= ~2.5e-7 (tests/test_gpu_parity.py::test_ann_tanh_accuracy);
// the limits come out exactly (e = inf -> 1, e = 0 -> -1) and NaN propagates.
// The r02 form sign(v) (1 - e') / (1 + e'), e' = exp2(-2 log2(e) |v|), needs a
// subtraction, a multiply and a sign copy more: tools/ubench.hip `act` measured
// 39.0 -> 35.5 cycles per element slot (-9 %), and exp2 from a degree-6 polynomial
// on the full-rate pipe (v_pk_fma_f32) instead of v_exp_f32 58.5 (+50 %: v_exp_f32
// issues in 8 cycles, the polynomial's range reduction, six packed fmas and
// exponent insert in more) -- profiles/r03/ubench.
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/ikhip.h"

namespace ikhip {

template <int ACT>
__device__ __forceinline__ float act_apply(float v) {
  if constexpr (ACT == IK_ACT_TANH) {
    const float e = __builtin_amdgcn_exp2f(2.885390081777927f * v);
    return __builtin_fmaf(-2.0f, __builtin_amdgcn_rcpf(1.0f + e), 1.0f);
  } else if constexpr (ACT == IK_ACT_RELU) {
    return v < 0.0f ? 0.0f : v;  // (fmaxf would turn NaN into 0)
  } else if constexpr (ACT == IK_ACT_SIGMOID) {
    return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.4426950408889634f * v));
  } else {
    return v;
  }
}

__device__ __forceinline__ float act_apply(int act, float v) {
  switch (act) {
    case IK_ACT_TANH:
      return act_apply<IK_ACT_TANH>(v);
    case IK_ACT_RELU:
      return act_apply<IK_ACT_RELU>(v);
    case IK_ACT_SIGMOID:
      return act_apply<IK_ACT_SIGMOID>(v);
    default:
      return v;
  }
}

// act' from the layer's stored output a = act(z)
__device__ __forceinline__ float act_deriv(int act, float a) {
  switch (act) {
    case IK_ACT_TANH:
      return 1.0f - a * a;
    case IK_ACT_RELU:
      return a > 0.0f ? 1.0f : 0.0f;
    case IK_ACT_SIGMOID:
      return a * (1.0f - a);
    default:
      return 1.0f;
  }
}

}  // namespace ikhip
