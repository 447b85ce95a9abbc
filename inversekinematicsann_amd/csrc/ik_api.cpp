// ik_api.cpp -- the C ABI of libikhip.so (declared in include/ikhip.h).
//
// Owns per-context state: the HIP stream, the device-side stats block, a
// grow-only device scratch buffer (host-pointer calls stage through it), the
// robot constants and the packed ANN weights.  No allocation happens inside a
// solve call once the scratch is large enough, so IK_F_DEVICE|IK_F_ASYNC calls
// can be captured in a hipGraph.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ik_analytic.h"
#include "ik_analytic_plan.h"
#include "ik_ann.h"
#include "ik_ann_pack.h"
#include "ik_fabrik.h"
#include "ik_fabrik_prior.h"
#include "ik_fk.h"
#include "ik_fk_chain.h"
#include "ik_internal.h"
#include "ik_launch.h"
#include "ik_refine.h"
#include "ik_types.h"

using namespace ikhip;

namespace {

thread_local std::string g_last_error;

const double kDefaultDh[16] = {0.0, kPi / 2, 0.0, 0.0, 2.0, 0.0, 0.0, 0.0,
                               0.0, 2.0,     2.0, 2.0, kPi / 2, 0.0, 0.0, 0.0};
const double kDefaultLinks[4] = {2.0, 2.0, 2.0, 2.0};
const double kDefaultLimits[6] = {0.0, 6.0, -6.0, 6.0, -3.0, 6.0};

thread_local KTimer *g_kt = nullptr;

static_assert(sizeof(FabPrior::key) == sizeof(FabOrderDev::key), "prior = one cost table");

// The FABRIK work order's built-in tables (ik_fabrik_prior.h) describe
// SixDOFRobot's chain (robot/robot.py:38-42): dh rows d, a, alpha and thetas[1:],
// and the links.  theta_1 (dh[0]) is never read on the device.
bool default_chain(const RobotDev &r) {
  return std::memcmp(r.dh + 1, kDefaultDh + 1, 15 * sizeof(double)) == 0 &&
         std::memcmp(r.links, kDefaultLinks, sizeof(kDefaultLinks)) == 0;
}

// The built-in table for a solve's (tol, max_iter): the nearest in log10(tol),
// then max_iter; -1 without one.
int prior_for(double tol, int max_iter) {
  int best = -1;
  double bd = 0.0;
  for (int k = 0; k < kFabPriors; ++k) {
    const double lt = tol > 0.0 ? std::log10(tol) : -30.0;
    const double d = std::fabs(lt - std::log10(kFabPrior[k].tol)) * 1000.0 +
                     std::fabs((double)(max_iter - kFabPrior[k].max_iter));
    if (best < 0 || d < bd) {
      best = k;
      bd = d;
    }
  }
  return best;
}

}  // namespace

namespace ikapi {

// A fresh table for the context's robot: the built-in one that suits (tol,
// max_iter) when the chain is SixDOFRobot's, else empty (point order).
int seed_order(ik_ctx *c, double tol, int max_iter) {
  const int w = (c->fab_priors && default_chain(c->robot)) ? prior_for(tol, max_iter) : -1;
  if (w >= 0)
    IK_HIP(hipMemcpyAsync(c->fab_ord->key, c->fab_priors + (size_t)w * kOrdCells,
                          sizeof(c->fab_ord->key), hipMemcpyDeviceToDevice, c->stream));
  else
    IK_HIP(hipMemsetAsync(c->fab_ord->key, 0, sizeof(c->fab_ord->key), c->stream));
  c->fab_prior = w;
  return IK_OK;
}

}  // namespace ikapi

namespace ikhip {
void kt_begin(const char *name, hipStream_t) {
  if (!g_kt || !g_kt->on || g_kt->n >= kMaxTimed) return;
  g_kt->name[g_kt->n] = name;
  g_kt->state = 1;
}
void kt_span_begin(const char *name, hipStream_t st) {
  if (!g_kt || !g_kt->on || g_kt->n >= kMaxTimed) return;
  g_kt->name[g_kt->n] = name;
  g_kt->state = 3;
  (void)hipEventRecord(g_kt->beg[g_kt->n], st);
}
bool kt_take_events(hipEvent_t *beg, hipEvent_t *end) {
  if (!g_kt || !g_kt->on || g_kt->n >= kMaxTimed || g_kt->state != 1) return false;
  *beg = g_kt->beg[g_kt->n];
  *end = g_kt->end[g_kt->n];
  g_kt->state = 2;
  return true;
}
void kt_end(hipStream_t st) {
  if (!g_kt || !g_kt->on || g_kt->n >= kMaxTimed) return;
  if (g_kt->state == 3) (void)hipEventRecord(g_kt->end[g_kt->n], st);
  // a slot armed without a stamped launch (no kernel ran) is dropped
  if (g_kt->state == 2 || g_kt->state == 3) g_kt->n++;
  g_kt->state = 0;
}
}  // namespace ikhip

namespace ikapi {

int fail(int code, const std::string &msg) {
  g_last_error = msg;
  return code;
}

KtScope::KtScope(ik_ctx *c) : c_(c) {
  g_kt = &c->kt;
  if (!c->kt.acc) c->kt.n = 0;  // (accumulating: slots fill across calls, up to kMaxTimed)
  c->kt.state = 0;
  // calls on one context share its stats block and work-queue words: a call on
  // another stream than the last one starts after that one's work
  if (c->call_done_set && c->last_stream && c->last_stream != c->stream)
    (void)hipStreamWaitEvent(c->stream, c->call_done, 0);
  c->last_stream = c->stream;  // every enqueueing entry point opens one
  c->last_piped = false;
}
KtScope::~KtScope() {
  g_kt = nullptr;
  if (c_->call_done && hipEventRecord(c_->call_done, c_->stream) == hipSuccess)
    c_->call_done_set = true;
}

int ensure_scratch(ik_ctx *c, size_t bytes) {
  if (bytes <= c->scratch_bytes) return IK_OK;
  IK_HIP(hipStreamSynchronize(c->stream));
  if (c->scratch) IK_HIP(hipFree(c->scratch));
  c->scratch = nullptr;
  c->scratch_bytes = 0;
  size_t want = bytes + bytes / 4 + (1 << 20);
  IK_HIP(hipMalloc(&c->scratch, want));
  c->scratch_bytes = want;
  return IK_OK;
}

int Stage::add(Kind kind, const void *user, size_t bytes) {
  if (n_ >= kMax) {  // refused by reserve()
    n_ = kMax + 1;
    return 0;
  }
  const bool staged = kind == kWork || kind == kTable || (!dev_ && (kind == kIn || user));
  r_[n_] = {kind, const_cast<void *>(user), bytes, staged ? cv_.add(bytes) : 0, staged, nullptr};
  return n_++;
}

int Stage::reserve() {
  if (n_ > kMax) return fail(IK_E_BADARG, "Stage: more than kMax regions");
  const int rc = ensure_scratch(c_, cv_.total);
  if (rc) return rc;
  for (Region *r = r_; r != r_ + n_; ++r) {
    r->dev = r->staged ? static_cast<char *>(c_->scratch) + r->off : r->user;
    if (r->staged && (r->kind == kTable || r->kind == kIn) && r->bytes)
      IK_HIP(hipMemcpyAsync(r->dev, r->user, r->bytes, hipMemcpyHostToDevice, c_->stream));
  }
  return IK_OK;
}

int Stage::flush() {
  for (const Region *r = r_; r != r_ + n_; ++r)
    if (r->staged && r->kind == kOut && r->bytes)
      IK_HIP(hipMemcpyAsync(r->user, r->dev, r->bytes, hipMemcpyDeviceToHost, c_->stream));
  return IK_OK;
}

int set_dev(ik_ctx *c) {
  IK_HIP(hipSetDevice(c->device));
  return IK_OK;
}

int check_flags(const char *who, int flags, const void *ang) {
  if (flags & IK_F_PITCH_NEAREST)  // (ik_analytic_solve clears it before it comes here)
    return fail(IK_E_BADARG, std::string(who) + ": IK_F_PITCH_NEAREST is ik_analytic_solve's");
  if ((flags & IK_F_ASYNC) && !(flags & IK_F_DEVICE))
    return fail(IK_E_BADARG, std::string(who) + ": IK_F_ASYNC requires IK_F_DEVICE");
  if ((flags & IK_F_DEVICE) && (reinterpret_cast<uintptr_t>(ang) & 15))
    return fail(IK_E_BADARG, std::string(who) + ": device ang must be 16-byte aligned");
  return IK_OK;
}

void stats_from_dev(const DevStats &d, ik_stats *s) {
  std::memset(s, 0, sizeof(*s));
  s->first_oob = (d.first_oob == ~0ull) ? -1 : (int64_t)d.first_oob;
  if (d.first_err_key == ~0ull) {
    s->first_err = -1;
    s->first_err_code = IK_OK;
  } else {
    s->first_err = (int64_t)(d.first_err_key >> 8);
    s->first_err_code = (int32_t)(d.first_err_key & 0xff);
  }
  for (int i = 0; i < kStatShards; ++i) {
    s->max_iters = d.max_iters[i] > s->max_iters ? d.max_iters[i] : s->max_iters;
    s->sum_iters += (int64_t)d.sum_iters[i];
    s->n_capped += (int64_t)d.n_capped[i];
    double mx;
    std::memcpy(&mx, &d.max_fk_err_bits[i], sizeof(mx));
    s->max_fk_err = mx > s->max_fk_err ? mx : s->max_fk_err;
    s->sum_fk_err += d.sum_fk_err[i];
  }
}

int finish(ik_ctx *c, int flags, ik_stats *stats) {
  c->last_sharded = false;
  if (flags & IK_F_ASYNC) return IK_OK;
  IK_HIP(hipMemcpyAsync(c->h_stats, c->d_stats, sizeof(DevStats), hipMemcpyDeviceToHost,
                        c->stream));
  IK_HIP(hipStreamSynchronize(c->stream));
  if (stats) stats_from_dev(*c->h_stats, stats);
  return IK_OK;
}

}  // namespace ikapi

using namespace ikapi;

namespace ikapi {

// Device pointers only, on the context's stream: stats reset + the kernels.
int fabrik_launch(ik_ctx *c, const double *dp, int64_t n, double tol, int max_iter, double *da,
                  int32_t *di, double *dj, double *dfe, bool limits, void *work, DevStats *S) {
  if (!S) S = c->d_stats;
  // a table still holding a built-in prior takes the one for this call's
  // tolerance; the solve then folds its own records in (learned from here on)
  const bool prior = c->fab_prior >= 0 && n > 0;
  if (prior) {
    if (prior_for(tol, max_iter) != c->fab_prior) {
      const int rc = seed_order(c, tol, max_iter);
      if (rc) return rc;
    }
    c->fab_prior = -1;
  }
  launch_reset_stats(S, c->stream);
  launch_fabrik_ikine(c->robot, dp, n, tol, max_iter, da, di, dj, dfe, limits, work, S,
                      c->stream, c->fabrik_variant, c->fabrik_core, c->fab_ord, c->rconst,
                      c->dbg, c->fabrik_bpc, prior);
  IK_HIP(hipGetLastError());
  return IK_OK;
}

int ann_launch(ik_ctx *c, const double *dp, int64_t n, float *da, double *de, bool limits,
               DevStats *S) {
  if (!S) S = c->d_stats;
  launch_reset_stats(S, c->stream);
  if (c->ann_big) {
    // two activation buffers of chunk x ld floats within IKHIP_ANN_ACT_MB (default
    // 1024 MiB; at least one 128-row tile), grown on demand
    if (n <= 0) return IK_OK;
    const char *bv = getenv("IKHIP_ANN_ACT_MB");  // (read per call: tests shrink it)
    long long budget_mb = (bv && *bv) ? atoll(bv) : 1024;
    if (budget_mb <= 0) budget_mb = 1024;
    const size_t ld = ann_big_ld(c->ann_bigm);
    int64_t rows = ann_big_rows(c->ann_bigm, (size_t)budget_mb << 20);
    if (rows < 128) rows = 128;
    const int64_t n128 = (n + 127) / 128 * 128;
    if (rows > n128) rows = n128;
    if (2 * (size_t)rows * ld * sizeof(float) > c->ann_act_bytes) {
      IK_HIP(hipStreamSynchronize(c->stream));
      if (c->ann_act) IK_HIP(hipFree(c->ann_act));
      c->ann_act = nullptr;
      c->ann_act_bytes = 0;
      // the budget's rows, or fewer (down to one 128-row tile, which ik_ann_load
      // checked would fit) when the device has less free
      for (;;) {
        const size_t bytes = 2 * (size_t)rows * ld * sizeof(float);
        const hipError_t e = hipMalloc(&c->ann_act, bytes);
        if (e == hipSuccess) {
          c->ann_act_bytes = bytes;
          break;
        }
        (void)hipGetLastError();
        if (e != hipErrorOutOfMemory || rows <= 128) IK_HIP(e);
        rows = (rows / 2 + 127) / 128 * 128;
      }
    }
    // the rows the buffers hold (a smaller earlier allocation limits the chunk)
    const int64_t fit = (int64_t)(c->ann_act_bytes / (2 * ld * sizeof(float))) / 128 * 128;
    if (rows > fit) rows = fit;
    // (both split modes run bf16x6 here: fp16x3's bounded-input planes are the
    // fused kernel's)
    launch_ann_big(c->ann_bigm, c->robot, dp, n, da, de, limits, S, c->stream,
                   static_cast<float *>(c->ann_act), rows, c->ann_mode);
    IK_HIP(hipGetLastError());
    return IK_OK;
  }
  AnnModelDev m = c->ann;
  m.xmode = c->ann_mode;
  for (int l = 0; l < m.n_layers; ++l) {
    m.wx[l] = c->ann_mode == IK_ANN_BF16X6   ? c->ann_wx[l]
              : c->ann_mode == IK_ANN_FP16X3 ? c->ann_wh[l]
                                             : nullptr;
    m.xinv[l] = c->ann_hinv[l];
  }
  launch_ann(m, c->robot, dp, n, da, de, limits, S, c->stream, c->dbg);
  IK_HIP(hipGetLastError());
  return IK_OK;
}

}  // namespace ikapi

extern "C" {

const char *ik_last_error(void) { return g_last_error.c_str(); }
const char *ik_version(void) { return "ikhip 0.1 gfx950"; }

int ik_ctx_create(int device, ik_ctx **out) {
  if (!out) return fail(IK_E_BADARG, "ik_ctx_create: out is NULL");
  *out = nullptr;
  int ndev = 0;
  IK_HIP(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev)
    return fail(IK_E_BADARG, "ik_ctx_create: device " + std::to_string(device) +
                                 " out of range (" + std::to_string(ndev) + " devices)");
  ik_ctx *c = new ik_ctx();
  c->device = device;
  int rc = set_dev(c);
  if (rc) {
    delete c;
    return rc;
  }
  hipError_t e = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipMalloc(&c->d_stats, sizeof(DevStats));
  if (e == hipSuccess) e = hipHostMalloc(&c->h_stats, sizeof(DevStats), hipHostMallocDefault);
  if (e == hipSuccess) e = hipMalloc(&c->fab_ord, sizeof(FabOrderDev));
  if (e == hipSuccess) e = hipMemset(c->fab_ord, 0, sizeof(FabOrderDev));
  if (e == hipSuccess && kFabPriors > 0) {
    e = hipMalloc(&c->fab_priors, sizeof(FabPrior::key) * kFabPriors);
    for (int k = 0; k < kFabPriors && e == hipSuccess; ++k)
      e = hipMemcpy(c->fab_priors + (size_t)k * kOrdCells, kFabPrior[k].key, sizeof(FabPrior::key),
                    hipMemcpyHostToDevice);
  }
  if (e == hipSuccess) e = hipMalloc(&c->rconst, sizeof(RobotConstDev));
  if (e == hipSuccess) e = hipEventCreateWithFlags(&c->call_done, hipEventDisableTiming);
  c->stream = c->own_stream;
  if (e != hipSuccess) {
    (void)ik_ctx_destroy(c);  // frees whatever was allocated
    return fail(IK_E_HIP, std::string("ik_ctx_create: ") + hipGetErrorString(e));
  }
  std::memcpy(c->robot.dh, kDefaultDh, sizeof(kDefaultDh));
  std::memcpy(c->robot.links, kDefaultLinks, sizeof(kDefaultLinks));
  std::memcpy(c->robot.lim, kDefaultLimits, sizeof(kDefaultLimits));
  launch_robot_const(c->robot, c->rconst, c->stream);
  // a fresh context's work order: SixDOFRobot's built-in table for the
  // reference's defaults (tol 1e-3, 100 iterations; FabrikInverseKinematics)
  if (seed_order(c, 1e-3, 100) != IK_OK) e = hipErrorUnknown;
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e == hipSuccess) e = hipGetLastError();
  if (e != hipSuccess) {
    (void)ik_ctx_destroy(c);
    return fail(IK_E_HIP, std::string("ik_ctx_create: ") + hipGetErrorString(e));
  }
  if (const char *v = std::getenv("IKHIP_FABRIK_VARIANT")) c->fabrik_variant = std::atoi(v);
  if (const char *v = std::getenv("IKHIP_FABRIK_CORE")) c->fabrik_core = std::atoi(v);
  if (const char *v = std::getenv("IKHIP_FABRIK_BPC")) c->fabrik_bpc = std::atoi(v);
  if (const char *v = std::getenv("IKHIP_ANN_MODE"))
    c->ann_mode = std::strcmp(v, "bf16x6") == 0   ? IK_ANN_BF16X6
                  : std::strcmp(v, "fp16x3") == 0 ? IK_ANN_FP16X3
                                                  : IK_ANN_FP32;
  *out = c;
  return IK_OK;
}

int ik_ctx_destroy(ik_ctx *c) {
  if (!c) return IK_OK;
  (void)hipSetDevice(c->device);
  // the communicator first: a live one's last call is waited for with its
  // deadline; an aborted one whose work has not drained leaves the context's
  // device memory to the process's end rather than block on it
  if (!comm_release(c)) return fail(IK_E_RCCL, "ik_ctx_destroy: aborted collective work has not "
                                               "drained; the context is left to the process's end");
  (void)hipStreamSynchronize(c->stream);
  if (c->scratch) (void)hipFree(c->scratch);
  if (c->ann_buf) (void)hipFree(c->ann_buf);
  if (c->ann_act) (void)hipFree(c->ann_act);
  train_release(c);
  if (c->d_stats) (void)hipFree(c->d_stats);
  if (c->dbg) (void)hipFree(c->dbg);
  if (c->fab_ord) (void)hipFree(c->fab_ord);
  if (c->fab_priors) (void)hipFree(c->fab_priors);
  if (c->rconst) (void)hipFree(c->rconst);
  if (c->h_stats) (void)hipHostFree(c->h_stats);
  pipe_release(c);
  if (c->call_done) (void)hipEventDestroy(c->call_done);
  if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
  for (int i = 0; i < kMaxTimed; ++i) {
    if (c->kt.beg[i]) (void)hipEventDestroy(c->kt.beg[i]);
    if (c->kt.end[i]) (void)hipEventDestroy(c->kt.end[i]);
  }
  delete c;
  return IK_OK;
}

int ik_ctx_set_stream(ik_ctx *c, void *stream) {
  if (!c) return fail(IK_E_BADARG, "ik_ctx_set_stream: NULL context");
  c->stream = stream ? static_cast<hipStream_t>(stream) : c->own_stream;
  return IK_OK;
}

void *ik_ctx_get_stream(ik_ctx *c) { return c ? static_cast<void *>(c->stream) : nullptr; }

int ik_set_robot(ik_ctx *c, const double *dh, const double *links, const double *limits) {
  if (!c) return fail(IK_E_BADARG, "ik_set_robot: NULL context");
  const RobotDev old = c->robot;
  if (dh) std::memcpy(c->robot.dh, dh, sizeof(c->robot.dh));
  if (links) std::memcpy(c->robot.links, links, sizeof(c->robot.links));
  if (limits) std::memcpy(c->robot.lim, limits, sizeof(c->robot.lim));
  // dh[0] (theta_1) is never read on the device: every solve takes the point's
  // own azimuth (inverse.py:123-125 writes it into the table per point), so a
  // drop-in caller re-sending the table with the last point's theta_1 changes
  // nothing.  The FABRIK cost table describes one chain (dh[1..15], links):
  // forget it only when that changes; the seed / limit constants follow any
  // change of those or of the limits.
  const bool chain = std::memcmp(old.dh + 1, c->robot.dh + 1, 15 * sizeof(double)) ||
                     std::memcmp(old.links, c->robot.links, sizeof(old.links));
  const bool lim = std::memcmp(old.lim, c->robot.lim, sizeof(old.lim)) != 0;
  if (chain || lim) {
    int rc = set_dev(c);
    if (rc) return rc;
    if (chain) {  // another chain's costs: its own (built-in for SixDOFRobot's), or empty
      const int rc = seed_order(c, 1e-3, 100);
      if (rc) return rc;
    }
    launch_robot_const(c->robot, c->rconst, c->stream);
    IK_HIP(hipGetLastError());
    // synchronous: later calls may run on another stream (ik_ctx_set_stream)
    IK_HIP(hipStreamSynchronize(c->stream));
  }
  return IK_OK;
}

int ik_ctx_set_timing(ik_ctx *c, int on) {
  if (!c) return fail(IK_E_BADARG, "ik_ctx_set_timing: NULL context");
  int rc = set_dev(c);
  if (rc) return rc;
  if (on && !c->kt.beg[0]) {
    for (int i = 0; i < kMaxTimed; ++i) {
      IK_HIP(hipEventCreate(&c->kt.beg[i]));
      IK_HIP(hipEventCreate(&c->kt.end[i]));
    }
  }
  c->kt.on = on != 0;
  c->kt.acc = on == 2;
  c->kt.n = 0;
  c->kt.state = 0;
  return IK_OK;
}

int ik_kernel_times(ik_ctx *c, int max, float *ms, char *names, int name_len) {
  if (!c || max < 0 || (max > 0 && !ms)) return -IK_E_BADARG;
  if (!c->kt.on) return 0;
  if (set_dev(c)) return -IK_E_HIP;
  int n = c->kt.n < max ? c->kt.n : max;
  for (int i = 0; i < n; ++i) {
    if (hipEventSynchronize(c->kt.end[i]) != hipSuccess) return -IK_E_HIP;
    float t = 0.0f;
    if (hipEventElapsedTime(&t, c->kt.beg[i], c->kt.end[i]) != hipSuccess) return -IK_E_HIP;
    ms[i] = t;
    if (names && name_len > 0) {
      std::strncpy(names + (size_t)i * name_len, c->kt.name[i], (size_t)name_len - 1);
      names[(size_t)i * name_len + name_len - 1] = 0;
    }
  }
  return n;
}

// the diagnostic buffer: ANN stamps or FABRIK iteration-kernel counters
static size_t debug_words() {
  return ann_debug_words() > kFabrikDebugWords ? ann_debug_words() : kFabrikDebugWords;
}

int ik_ctx_set_debug(ik_ctx *c, int on) {
  if (!c) return fail(IK_E_BADARG, "ik_ctx_set_debug: NULL context");
  int rc = set_dev(c);
  if (rc) return rc;
  IK_HIP(hipStreamSynchronize(c->stream));
  if (on && !c->dbg) {
    IK_HIP(hipMalloc(&c->dbg, debug_words() * 8));
    IK_HIP(hipMemset(c->dbg, 0, debug_words() * 8));
  } else if (!on && c->dbg) {
    IK_HIP(hipFree(c->dbg));
    c->dbg = nullptr;
  }
  return IK_OK;
}

int ik_debug_read(ik_ctx *c, uint64_t *out, int max) {
  if (!c || !out || max < 0) return -IK_E_BADARG;
  if (!c->dbg) return 0;
  if (set_dev(c)) return -IK_E_HIP;
  int n = (int)debug_words() < max ? (int)debug_words() : max;
  if (hipStreamSynchronize(c->stream) != hipSuccess) return -IK_E_HIP;
  if (hipMemcpy(out, c->dbg, (size_t)n * 8, hipMemcpyDeviceToHost) != hipSuccess)
    return -IK_E_HIP;
  return n;
}

int ik_ctx_sync(ik_ctx *c) {
  if (!c) return fail(IK_E_BADARG, "ik_ctx_sync: NULL context");
  int rc = set_dev(c);
  if (rc) return rc;
  if (c->last_piped) return IK_OK;  // a chunked host pipeline returns complete
  if (!c->call_done_set) return IK_OK;
  // with a communicator the wait is bounded (its deadline and async errors)
  rc = comm_wait(c, c->call_done, "the last call");
  if (rc) return rc;
  // an IK_F_ASYNC sharded call is validated here as ik_stats_fetch would: every
  // rank planned the same (n, chunks, method), else the gathered rows belong to
  // another plan
  if (c->last_sharded) return sharded_stats(c, nullptr);
  return IK_OK;
}

int ik_stats_fetch(ik_ctx *c, ik_stats *stats) {
  if (!c) return fail(IK_E_BADARG, "ik_stats_fetch: NULL context");
  int rc = set_dev(c);
  if (rc) return rc;
  // the stats of the last call live on the stream it ran on (ik_ctx_set_stream may
  // have switched since)
  if (c->last_piped) {  // a chunked host pipeline: merged when it returned
    if (stats) *stats = c->piped_stats;
    return IK_OK;
  }
  hipStream_t cur = c->stream;
  if (c->last_stream) c->stream = c->last_stream;
  rc = c->last_sharded ? sharded_stats(c, stats) : finish(c, 0, stats);
  c->stream = cur;
  return rc;
}

int ik_check_limits(ik_ctx *c, const double *pts, int64_t n, int flags, ik_stats *stats) {
  if (!c || n < 0 || (n > 0 && !pts)) return fail(IK_E_BADARG, "ik_check_limits: bad args");
  int rc = check_flags("ik_check_limits", flags);
  if (rc || (rc = set_dev(c))) return rc;
  KtScope kts(c);
  Stage st(c, flags);
  const int r_pts = st.in(pts, (size_t)n * 24);
  if ((rc = st.reserve())) return rc;
  launch_reset_stats(c->d_stats, c->stream);
  launch_check_limits(c->robot, st.at<const double>(r_pts), n, c->d_stats, c->stream);
  IK_HIP(hipGetLastError());
  return finish(c, flags, stats);
}

// ---- joint limits (honoured by the refine: ik_refine.hip) -----------------------
int ik_set_joint_limits(ik_ctx *c, const double *lo, const double *hi) {
  if (!c) return fail(IK_E_BADARG, "ik_set_joint_limits: NULL context");
  if (!lo != !hi)
    return fail(IK_E_BADARG, "ik_set_joint_limits: lo and hi must both be given or both be NULL");
  JointLimits jl = {{-HUGE_VAL, -HUGE_VAL, -HUGE_VAL, -HUGE_VAL},
                    {HUGE_VAL, HUGE_VAL, HUGE_VAL, HUGE_VAL}, 0u};
  for (int i = 0; lo && i < 4; ++i) {
    const std::string who = "ik_set_joint_limits: joint " + std::to_string(i + 1) + ": ";
    if (std::isnan(lo[i]) || std::isnan(hi[i])) return fail(IK_E_BADARG, who + "a bound is NaN");
    if (lo[i] == -HUGE_VAL && hi[i] == HUGE_VAL) continue;  // free
    if (std::isinf(lo[i]) != std::isinf(hi[i]))
      return fail(IK_E_BADARG, who + "one bound is infinite and the other finite");
    if (lo[i] > hi[i]) return fail(IK_E_BADARG, who + "lo > hi");
    if (lo[i] < -kPi || hi[i] > kPi)
      return fail(IK_E_BADARG, who + "a bound lies outside [-pi, pi]");
    jl.lo[i] = lo[i];
    jl.hi[i] = hi[i];
    jl.mask |= 1u << i;
  }
  c->jlim = jl;
  return IK_OK;
}

int ik_get_joint_limits(ik_ctx *c, double *lo, double *hi) {
  if (!c || !lo || !hi) return fail(IK_E_BADARG, "ik_get_joint_limits: bad args");
  std::memcpy(lo, c->jlim.lo, sizeof(c->jlim.lo));
  std::memcpy(hi, c->jlim.hi, sizeof(c->jlim.hi));
  return IK_OK;
}

int ik_check_joint_limits(ik_ctx *c, const double *ang, int64_t n, int flags, ik_stats *stats) {
  if (!c || n < 0 || (n > 0 && !ang)) return fail(IK_E_BADARG, "ik_check_joint_limits: bad args");
  int rc = check_flags("ik_check_joint_limits", flags, ang);
  if (rc || (rc = set_dev(c))) return rc;
  KtScope kts(c);
  Stage st(c, flags);
  const int r_ang = st.in(ang, (size_t)n * 32);
  if ((rc = st.reserve())) return rc;
  launch_reset_stats(c->d_stats, c->stream);
  launch_check_joint_limits(c->jlim, st.at<const double>(r_ang), n, c->d_stats, c->stream);
  IK_HIP(hipGetLastError());
  return finish(c, flags, stats);
}

int ik_fk(ik_ctx *c, const double *ang, int64_t n, double *xyz, double *mats, int flags,
          ik_stats *stats) {
  if (!c || n < 0 || (n > 0 && (!ang || !xyz))) return fail(IK_E_BADARG, "ik_fk: bad args");
  int rc = check_flags("ik_fk", flags);
  if (rc || (rc = set_dev(c))) return rc;
  KtScope kts(c);
  Stage st(c, flags);
  const int r_ang = st.in(ang, (size_t)n * 32), r_xyz = st.out(xyz, (size_t)n * 24),
            r_mats = st.out(mats, (size_t)n * 512);  // n x 4 x 16
  if ((rc = st.reserve())) return rc;
  launch_reset_stats(c->d_stats, c->stream);
  launch_fk(c->robot, st.at<const double>(r_ang), n, st.at<double>(r_xyz),
            st.at<double>(r_mats), c->d_stats, c->stream);
  IK_HIP(hipGetLastError());
  if ((rc = st.flush())) return rc;
  return finish(c, flags, stats);
}

int ik_fk_chain(ik_ctx *c, int nj, const double *dh, const double *ang, int64_t n,
                double *xyz, double *mats, int flags, ik_stats *stats) {
  if (!c || nj < 2 || nj > kFkMaxJoints || !dh || n < 0 || (n > 0 && (!ang || !xyz)))
    return fail(IK_E_BADARG, "ik_fk_chain: bad args (nj must be 2.." +
                                 std::to_string(kFkMaxJoints) + ")");
  int rc = check_flags("ik_fk_chain", flags);
  if (rc || (rc = set_dev(c))) return rc;
  KtScope kts(c);
  Stage st(c, flags);
  const int r_dh = st.table(dh, (size_t)nj * 32), r_ang = st.in(ang, (size_t)n * nj * 8),
            r_xyz = st.out(xyz, (size_t)n * 24), r_mats = st.out(mats, (size_t)n * nj * 128);
  if ((rc = st.reserve())) return rc;
  launch_reset_stats(c->d_stats, c->stream);
  launch_fk_n(nj, st.at<const double>(r_dh), st.at<const double>(r_ang), n, st.at<double>(r_xyz),
              st.at<double>(r_mats), c->d_stats, c->stream);
  IK_HIP(hipGetLastError());
  if ((rc = st.flush())) return rc;
  // dh came from a host buffer that may go away: always complete before return
  if (flags & IK_F_ASYNC) IK_HIP(hipStreamSynchronize(c->stream));
  return finish(c, flags, stats);
}

int ik_fabrik_solve(ik_ctx *c, const double *pts, int64_t n, double tol, int32_t max_iter,
                    double *ang, int32_t *iters, double *joints, int flags, ik_stats *stats) {
  return ik_fabrik_solve_fk(c, pts, n, tol, max_iter, ang, iters, joints, nullptr, flags, stats);
}

int ik_fabrik_solve_fk(ik_ctx *c, const double *pts, int64_t n, double tol, int32_t max_iter,
                       double *ang, int32_t *iters, double *joints, double *fk_err, int flags,
                       ik_stats *stats) {
  if (!c || n < 0 || (n > 0 && (!pts || !ang)) || max_iter < 0)
    return fail(IK_E_BADARG, "ik_fabrik_solve: bad args");
  int rc = check_flags("ik_fabrik_solve", flags, ang);
  if (rc || (rc = set_dev(c))) return rc;
  KtScope kts(c);
  if (!(flags & IK_F_DEVICE) && pipeline_wanted(c, n, {pts, ang, iters, joints, fk_err}))
    return fabrik_host_pipeline(c, pts, n, tol, max_iter, ang, iters, joints, fk_err, flags,
                                stats);
  Stage st(c, flags);
  const int r_work = st.work(fabrik_scratch_bytes(n)), r_pts = st.in(pts, (size_t)n * 24),
            r_ang = st.out(ang, (size_t)n * 32), r_it = st.out(iters, (size_t)n * 4),
            r_jo = st.out(joints, (size_t)n * 96), r_fe = st.out(fk_err, (size_t)n * 8);
  if ((rc = st.reserve())) return rc;
  rc = fabrik_launch(c, st.at<const double>(r_pts), n, tol, max_iter, st.at<double>(r_ang),
                     st.at<int32_t>(r_it), st.at<double>(r_jo), st.at<double>(r_fe),
                     !(flags & IK_F_NO_LIMITS), st.at<void>(r_work));
  if (rc || (rc = st.flush())) return rc;
  return finish(c, flags, stats);
}

int ik_fabrik_reset_order(ik_ctx *c) {
  if (!c) return fail(IK_E_BADARG, "ik_fabrik_reset_order: NULL context");
  int rc = set_dev(c);
  if (rc) return rc;
  KtScope kts(c);  // ordered after the context's earlier calls, whatever their stream
  return seed_order(c, 1e-3, 100);
}

int ik_fabrik_order_get(ik_ctx *c, uint32_t *key, int n) {
  if (!c || !key || n < kOrdCells) return -fail(IK_E_BADARG, "ik_fabrik_order_get: bad args");
  if (set_dev(c)) return -IK_E_HIP;
  // the last call's end, waited for with the communicator's deadline when one is
  // bound (a dead peer ends the wait with IK_E_RCCL instead of hanging it)
  if (c->call_done_set) {
    const int rc = comm_wait(c, c->call_done, "the last call");
    if (rc) return -rc;
  } else if (hipStreamSynchronize(c->stream) != hipSuccess) {
    return -fail(IK_E_HIP, "ik_fabrik_order_get: stream synchronize failed");
  }
  if (hipMemcpy(key, c->fab_ord->key, sizeof(c->fab_ord->key), hipMemcpyDeviceToHost) != hipSuccess)
    return -fail(IK_E_HIP, "ik_fabrik_order_get: copy failed");
  return kOrdCells;
}

int ik_fabrik_order_set(ik_ctx *c, const uint32_t *key, int n) {
  if (!c || (key && n != kOrdCells)) return fail(IK_E_BADARG, "ik_fabrik_order_set: bad args");
  int rc = set_dev(c);
  if (rc) return rc;
  KtScope kts(c);
  IK_HIP(hipStreamSynchronize(c->stream));  // key may be a short-lived host buffer
  if (key)
    IK_HIP(hipMemcpy(c->fab_ord->key, key, sizeof(c->fab_ord->key), hipMemcpyHostToDevice));
  else
    IK_HIP(hipMemset(c->fab_ord->key, 0, sizeof(c->fab_ord->key)));
  c->fab_prior = -1;
  return IK_OK;
}

int ik_fabrik_calc(ik_ctx *c, int nj, const double *dists, const double *init,
                   int init_shared, const double *goals, int64_t n, double tol,
                   int32_t max_iter, double *joints, int32_t *iters, int flags,
                   ik_stats *stats) {
  if (!c || nj < 1 || nj > kCalcMaxJoints || !dists || n < 0 ||
      (n > 0 && (!init || !goals || !joints)) || max_iter < 0)
    return fail(IK_E_BADARG, "ik_fabrik_calc: bad args (nj must be 1.." +
                                 std::to_string(kCalcMaxJoints) + ")");
  int rc = check_flags("ik_fabrik_calc", flags);
  if (rc || (rc = set_dev(c))) return rc;
  KtScope kts(c);
  Stage st(c, flags);
  const size_t n_init = init_shared ? (size_t)nj * 3 : (size_t)n * nj * 3;
  const int r_d = st.table(dists, (size_t)nj * 8), r_init = st.in(init, n_init * 8),
            r_g = st.in(goals, (size_t)n * 24), r_jo = st.out(joints, (size_t)n * nj * 24),
            r_it = st.out(iters, (size_t)n * 4);
  if ((rc = st.reserve())) return rc;
  launch_reset_stats(c->d_stats, c->stream);
  launch_fabrik_calc(nj, st.at<const double>(r_d), st.at<const double>(r_init), init_shared != 0,
                     st.at<const double>(r_g), n, tol, max_iter, st.at<double>(r_jo),
                     st.at<int32_t>(r_it), c->d_stats, c->stream);
  IK_HIP(hipGetLastError());
  if ((rc = st.flush())) return rc;
  // dists came from a host buffer that may go away: always complete before return
  if (flags & IK_F_ASYNC) IK_HIP(hipStreamSynchronize(c->stream));
  return finish(c, flags, stats);
}

int ik_ann_load(ik_ctx *c, int n_layers, const int32_t *dims, const int32_t *acts,
                const float *const *W, const float *const *b, const double *x_mean,
                const double *x_scale, const double *y_mean, const double *y_scale) {
  if (!c || n_layers < 1 || n_layers > kAnnBigMaxLayers || !dims || !acts || !W || !b ||
      !x_mean || !x_scale || !y_mean || !y_scale)
    return fail(IK_E_BADARG, "ik_ann_load: bad args (1.." + std::to_string(kAnnBigMaxLayers) +
                                 " layers)");
  if (dims[0] != 3 || dims[n_layers] != 4)
    return fail(IK_E_BADARG, "ik_ann_load: the model must map 3 inputs to 4 outputs");
  for (int l = 0; l <= n_layers; ++l)
    if (dims[l] < 1 || dims[l] > kAnnBigMaxWidth)
      return fail(IK_E_BADARG, "ik_ann_load: layer widths must be 1.." +
                                   std::to_string(kAnnBigMaxWidth));
  for (int l = 0; l < n_layers; ++l)
    if (acts[l] < IK_ACT_LINEAR || acts[l] > IK_ACT_SIGMOID)
      return fail(IK_E_BADARG, "ik_ann_load: unsupported activation code");
  int rc = set_dev(c);
  if (rc) return rc;
  // one device buffer, per layer a section of packed weights, padded bias and
  // the split modes' operands where the layer can take them (AnnLayout)
  AnnLayout L(n_layers, dims, acts, true);
  // (the widths and depth are capped above, so `total` stays far below 2^64: at
  // most 4096 layers of a 16384 x 16384 product, ~4.4 TB -- but that may not fit
  // the device, and the host staging must not be one buffer of that size)
  IK_HIP(hipStreamSynchronize(c->stream));
  if (c->ann_buf) IK_HIP(hipFree(c->ann_buf));
  c->ann_buf = nullptr;
  c->ann_loaded = false;
  size_t dev_free = 0, dev_total = 0;
  IK_HIP(hipMemGetInfo(&dev_free, &dev_total));
  // the layered path's first solve also needs its two activation buffers: at
  // least one 128-row tile of the widest padded layer (ann_launch takes up to
  // IKHIP_ANN_ACT_MB and falls back to fewer rows when that much is not free;
  // ADVICE r05), less what a previous model's buffers already hold
  const size_t act_min = L.act_min > c->ann_act_bytes ? L.act_min - c->ann_act_bytes : 0;
  // without the split planes?  (a split mode then runs fp32: ik_ann_effective_mode says so)
  if (L.total + act_min > dev_free) L = AnnLayout(n_layers, dims, acts, false);
  if (L.total + act_min > dev_free)
    return fail(IK_E_HIP, "ik_ann_load: the packed model needs " + std::to_string(L.total) +
                              " bytes of device memory (+ " + std::to_string(act_min) +
                              " for its activations), " + std::to_string(dev_free) +
                              " are free");
  IK_HIP(hipMalloc(&c->ann_buf, L.total));
  char *base = static_cast<char *>(c->ann_buf);
  // pack and upload one layer's section at a time: the host holds
  // at most the largest layer's packed bytes, and an allocation failure is an
  // error code, not an exception leaving the C ABI
  std::vector<int> hexp(n_layers, 0);
  std::vector<char> hbuilt(n_layers, 0);
  try {
    std::vector<char> host;
    for (int l = 0; l < n_layers; ++l) {
      host.assign(L.section_bytes(l), 0);
      bool built = false;
      hexp[l] = ann_pack_section(L, l, W[l], b[l], host.data(), &built);
      hbuilt[l] = built;
      IK_HIP(hipMemcpy(base + L.woff[l], host.data(), host.size(), hipMemcpyHostToDevice));
    }
  } catch (const std::bad_alloc &) {
    (void)hipFree(c->ann_buf);
    c->ann_buf = nullptr;
    return fail(IK_E_HIP, "ik_ann_load: out of host memory staging the packed weights");
  }
  c->ann_big = L.big;
  AnnBigModel &bm = c->ann_bigm;
  AnnModelDev &m = c->ann;
  bm.layers.clear();
  std::memset(&m, 0, sizeof(m));
  m.n_layers = L.big ? 0 : n_layers;
  std::copy(x_mean, x_mean + 3, L.big ? bm.xm : m.xm);
  std::copy(x_scale, x_scale + 3, L.big ? bm.xs : m.xs);
  std::copy(y_mean, y_mean + 4, L.big ? bm.ym : m.ym);
  std::copy(y_scale, y_scale + 4, L.big ? bm.ys : m.ys);
  for (int l = 0; l < n_layers; ++l) {
    const float *wp = reinterpret_cast<const float *>(base + L.woff[l]);
    const float *bias = reinterpret_cast<const float *>(base + L.boff[l]);
    const char *wx = L.splittable[l] ? base + L.xoff[l] : nullptr;
    if (L.big) {
      bm.layers.push_back({L.kp(l), L.np(l), acts[l], wp, bias,
                           reinterpret_cast<const uint16_t *>(wx)});
      continue;
    }
    m.kp[l] = L.kp(l);
    m.np[l] = L.np(l);
    m.act[l] = acts[l];
    m.wp[l] = reinterpret_cast<const float4 *>(wp);
    m.bias[l] = bias;
    c->ann_wx[l] = wx;
    // (no planes for a layer whose weights are out of the pre-scale's range: fp32)
    c->ann_wh[l] = hbuilt[l] ? base + L.hoff[l] : nullptr;
    c->ann_hinv[l] = std::ldexp(1.0f, -hexp[l]);
  }
  c->ann_loaded = true;
  return IK_OK;
}

int ik_ann_set_mode(ik_ctx *c, int mode) {
  if (!c) return fail(IK_E_BADARG, "ik_ann_set_mode: NULL context");
  if (mode != IK_ANN_FP32 && mode != IK_ANN_BF16X6 && mode != IK_ANN_FP16X3)
    return fail(IK_E_BADARG, "ik_ann_set_mode: unknown mode");
  c->ann_mode = mode;
  return IK_OK;
}

int ik_ann_get_mode(ik_ctx *c) { return c ? c->ann_mode : -IK_E_BADARG; }

int ik_ann_effective_mode(ik_ctx *c) {
  if (!c) return -IK_E_BADARG;
  if (!c->ann_loaded) return -fail(IK_E_NOMODEL, "ik_ann_effective_mode: no model loaded");
  if (c->ann_mode == IK_ANN_FP32) return IK_ANN_FP32;
  if (c->ann_big) {  // both split modes run bf16x6 there
    for (const AnnBigLayer &L : c->ann_bigm.layers)
      if (L.wx) return IK_ANN_BF16X6;
    return IK_ANN_FP32;
  }
  const void *const *ops = c->ann_mode == IK_ANN_BF16X6 ? c->ann_wx : c->ann_wh;
  for (int l = 0; l < c->ann.n_layers; ++l)
    if (ops[l]) return c->ann_mode;
  return IK_ANN_FP32;
}

int ik_ann_solve(ik_ctx *c, const double *pts, int64_t n, float *ang, double *fk_err,
                 int flags, ik_stats *stats) {
  if (!c || n < 0 || (n > 0 && (!pts || !ang))) return fail(IK_E_BADARG, "ik_ann_solve: bad args");
  if (!c->ann_loaded) return fail(IK_E_NOMODEL, "ik_ann_solve: no model loaded (ik_ann_load)");
  int rc = check_flags("ik_ann_solve", flags, ang);
  if (rc || (rc = set_dev(c))) return rc;
  KtScope kts(c);
  // (no chunked pipeline for ANN: its copies are ~2 % of the call and splitting
  // the launch into chunks costs more tile-quantisation tail than the overlap
  // saves -- 41.6 vs 41.1 ms per 1M points measured)
  Stage st(c, flags);
  const int r_pts = st.in(pts, (size_t)n * 24), r_ang = st.out(ang, (size_t)n * 16),
            r_fe = st.out(fk_err, (size_t)n * 8);
  if ((rc = st.reserve())) return rc;
  rc = ann_launch(c, st.at<const double>(r_pts), n, st.at<float>(r_ang), st.at<double>(r_fe),
                  !(flags & IK_F_NO_LIMITS));
  if (rc || (rc = st.flush())) return rc;
  return finish(c, flags, stats);
}

// ---- refine (ik_refine.hip) ----------------------------------------------------
}  // extern "C"

int ikapi::refine_args(const char *who, ik_ctx *c, int64_t n, bool arrays, double tol,
                       int32_t max_iter, double damping, const double *ang, int flags) {
  const std::string w(who);
  if (!c || n < 0 || (n > 0 && !arrays) || max_iter < 0) return fail(IK_E_BADARG, w + ": bad args");
  if (std::isnan(tol)) return fail(IK_E_BADARG, w + ": tol is NaN");
  if (!std::isfinite(damping) || !(damping > 0.0))
    return fail(IK_E_BADARG, w + ": damping must be finite and > 0");
  return check_flags(who, flags, ang);
}

extern "C" {

int ik_refine(ik_ctx *c, const double *pts, const double *seed, int64_t n, double tol,
              int32_t max_iter, double damping, double *ang, int32_t *iters, double *fk_err,
              int flags, ik_stats *stats) {
  int rc = refine_args("ik_refine", c, n, pts && seed && ang, tol, max_iter, damping, ang, flags);
  if (rc || (rc = set_dev(c))) return rc;
  KtScope kts(c);
  Stage st(c, flags);
  const int r_pts = st.in(pts, (size_t)n * 24), r_seed = st.in(seed, (size_t)n * 32),
            r_ang = st.out(ang, (size_t)n * 32), r_it = st.out(iters, (size_t)n * 4),
            r_fe = st.out(fk_err, (size_t)n * 8);
  if ((rc = st.reserve())) return rc;
  launch_reset_stats(c->d_stats, c->stream);
  launch_refine(c->rconst, st.at<const double>(r_pts), st.at<const double>(r_seed), n, tol,
                max_iter, damping, st.at<double>(r_ang), st.at<int32_t>(r_it),
                st.at<double>(r_fe), !(flags & IK_F_NO_LIMITS), c->jlim, c->d_stats, c->stream);
  IK_HIP(hipGetLastError());
  if ((rc = st.flush())) return rc;
  return finish(c, flags, stats);
}

int ik_ann_solve_refined(ik_ctx *c, const double *pts, int64_t n, double tol, int32_t max_iter,
                         double damping, double *ang, int32_t *iters, double *fk_err,
                         double *seed_fk_err, int flags, ik_stats *stats) {
  int rc = refine_args("ik_ann_solve_refined", c, n, pts && ang, tol, max_iter, damping, ang,
                       flags);
  if (rc) return rc;
  if (!c->ann_loaded)
    return fail(IK_E_NOMODEL, "ik_ann_solve_refined: no model loaded (ik_ann_load)");
  if ((rc = set_dev(c))) return rc;
  KtScope kts(c);
  const bool limits = !(flags & IK_F_NO_LIMITS);
  Stage st(c, flags);
  // the network's float32 angles never leave the device: they are the refine's seeds
  const int r_seed = st.work((size_t)n * 16), r_pts = st.in(pts, (size_t)n * 24),
            r_ang = st.out(ang, (size_t)n * 32), r_it = st.out(iters, (size_t)n * 4),
            r_fe = st.out(fk_err, (size_t)n * 8), r_se = st.out(seed_fk_err, (size_t)n * 8);
  if ((rc = st.reserve())) return rc;
  const double *dp = st.at<const double>(r_pts);
  float *dseed = st.at<float>(r_seed);
  if ((rc = ann_launch(c, dp, n, dseed, st.at<double>(r_se), limits))) return rc;
  // the call's stats are the refined result's
  launch_reset_stats(c->d_stats, c->stream);
  launch_refine_f32(c->rconst, dp, dseed, n, tol, max_iter, damping, st.at<double>(r_ang),
                    st.at<int32_t>(r_it), st.at<double>(r_fe), limits, c->jlim, c->d_stats,
                    c->stream);
  IK_HIP(hipGetLastError());
  if ((rc = st.flush())) return rc;
  return finish(c, flags, stats);
}

// ---- analytic (ik_analytic.hip) ------------------------------------------------
int ik_analytic_solve(ik_ctx *c, const double *pts, const double *pitch, int64_t n, int elbow,
                      double *ang, double *pitch_out, double *fk_err, int flags, ik_stats *stats) {
  if (!c || n < 0 || (n > 0 && (!pts || !ang)))
    return fail(IK_E_BADARG, "ik_analytic_solve: bad args");
  if (elbow != IK_ELBOW_UP && elbow != IK_ELBOW_DOWN)
    return fail(IK_E_BADARG, "ik_analytic_solve: elbow " + std::to_string(elbow) +
                                 " is neither IK_ELBOW_UP (-1) nor IK_ELBOW_DOWN (1)");
  const bool nearest = flags & IK_F_PITCH_NEAREST;
  flags &= ~IK_F_PITCH_NEAREST;  // (the one call that takes the bit)
  int rc = check_flags("ik_analytic_solve", flags, ang);
  if (rc) return rc;
  AnalyticRobot robot;  // (the kernel reads the same lengths from the robot constants)
  const std::string why = analytic_robot(c->robot.dh, &robot);
  if (!why.empty())
    return fail(IK_E_BADARG, "ik_analytic_solve: the robot is not a yaw joint + planar "
                             "three-link chain: " + why);
  if ((rc = set_dev(c))) return rc;
  KtScope kts(c);
  Stage st(c, flags);
  const int r_pts = st.in(pts, (size_t)n * 24), r_ph = pitch ? st.in(pitch, (size_t)n * 8) : -1,
            r_ang = st.out(ang, (size_t)n * 32), r_po = st.out(pitch_out, (size_t)n * 8),
            r_fe = st.out(fk_err, (size_t)n * 8);
  if ((rc = st.reserve())) return rc;
  launch_reset_stats(c->d_stats, c->stream);
  launch_analytic(c->rconst, st.at<const double>(r_pts),
                  r_ph < 0 ? nullptr : st.at<const double>(r_ph), n, elbow, nearest,
                  st.at<double>(r_ang), st.at<double>(r_po), st.at<double>(r_fe),
                  !(flags & IK_F_NO_LIMITS), c->d_stats, c->stream);
  IK_HIP(hipGetLastError());
  if ((rc = st.flush())) return rc;
  return finish(c, flags, stats);
}

}  // extern "C"
