// ik_launch.h -- what the host side of every launcher shares: the robot as the
// kernels take it, the timed launch (kt_begin / IK_LAUNCH / kt_end) and the
// device's CU count.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <atomic>
#include <cmath>

#include "ik_types.h"

namespace ikhip {
struct RobotDev {
  double dh[16];
  double links[4];
  double lim[6];
};

// Host: the per-joint constants of fk_error, {a_i, d_i, cos alpha_i, sin alpha_i},
// and whether some |alpha_i| > 2 pi (then FK raises for every point, forward.py:23-25).
inline void fk_trip_consts(const RobotDev &r, double jc[16], int *alpha_bad) {
  *alpha_bad = 0;
  for (int i = 0; i < 4; ++i) {
    const double al = r.dh[12 + i];
    jc[4 * i + 0] = r.dh[8 + i];
    jc[4 * i + 1] = r.dh[4 + i];
    jc[4 * i + 2] = std::cos(al);
    jc[4 * i + 3] = std::sin(al);
    if (al < -2 * kPi || al > 2 * kPi) *alpha_bad = 1;
  }
}

// Optional per-kernel HIP-event timing of the current call (ik_ctx_set_timing):
// launchers bracket every kernel with kt_begin / IK_LAUNCH / kt_end.  The kernel's
// events are handed to hipExtLaunchKernel, so the dispatch itself stamps its own
// start and end: neither the kernels ahead of it on the stream nor the host's
// launch latency fall inside the interval.  Spans that are not
// one kernel (the RCCL gather) use kt_span_begin: stream markers.
void kt_begin(const char *name, hipStream_t st);
void kt_span_begin(const char *name, hipStream_t st);
void kt_end(hipStream_t st);
// the armed slot's events for the kernel about to launch (false: timing is off)
bool kt_take_events(hipEvent_t *beg, hipEvent_t *end);
#define IK_LAUNCH(K, G, B, SH, ST, ...)                                             \
  do {                                                                              \
    hipEvent_t ik_kb_ = nullptr, ik_ke_ = nullptr;                                  \
    if (::ikhip::kt_take_events(&ik_kb_, &ik_ke_))                                  \
      hipExtLaunchKernelGGL(K, G, B, SH, ST, ik_kb_, ik_ke_, 0u, __VA_ARGS__);      \
    else                                                                            \
      hipLaunchKernelGGL(K, G, B, SH, ST, __VA_ARGS__);                             \
  } while (0)

// CUs of the current device, cached per device index (relaxed atomics: every
// writer stores the same value)
inline int num_cus() {
  static std::atomic<int> cache[64];
  int dev = 0;
  (void)hipGetDevice(&dev);
  std::atomic<int> *slot = (dev >= 0 && dev < 64) ? &cache[dev] : nullptr;
  int v = slot ? slot->load(std::memory_order_relaxed) : 0;
  if (v <= 0) {
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        v <= 0)
      v = 256;
    if (slot) slot->store(v, std::memory_order_relaxed);
  }
  return v;
}

}  // namespace ikhip
