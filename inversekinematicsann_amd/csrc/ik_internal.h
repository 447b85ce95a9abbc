// ik_internal.h -- the context behind the C ABI and the helpers its
// translation units share (ik_api.cpp: single-device calls; ik_pipe.cpp: the
// chunked host-pointer pipeline; ik_train_api.cpp: the training calls, whose
// layouts / epoch plan / refusals are the host-only ik_train_plan.cpp;
// ik_chain_api.cpp: ik_chain_solve; ik_shard.hip: the RCCL-sharded calls, whose plan / tail / histogram arithmetic
// is the host-only ik_shard_plan.cpp).  Not installed; include/ikhip.h is the
// interface.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <initializer_list>
#include <string>

#include "../../include/ikhip.h"
#include "ik_ann.h"
#include "ik_ann_pack.h"
#include "ik_fabrik.h"
#include "ik_launch.h"
#include "ik_refine_step.h"
#include "ik_train.h"
#include "ik_types.h"

namespace ikhip {
constexpr int kMaxTimed = 64;  // kernels timed per call (the layered ANN path launches one per layer)
struct KTimer {
  bool on = false;
  bool acc = false;  // ik_ctx_set_timing(ctx, 2): the calls' kernels accumulate
  int n = 0;
  // slot n's state: 1 = armed by kt_begin (the next IK_LAUNCH takes its events),
  // 2 = stamped by that dispatch, 3 = a marker span (kt_span_begin)
  int state = 0;
  hipEvent_t beg[kMaxTimed] = {};
  hipEvent_t end[kMaxTimed] = {};
  const char *name[kMaxTimed] = {};
};
}  // namespace ikhip

// What a rank planned its sharded call with; every rank's must agree (a rank
// that planned another batch or chunk count gathered other rows).
struct IkPlanHdr {
  int64_t n;
  int32_t chunks, method;
  uint32_t magic, pad;
};
constexpr uint32_t kPlanMagic = 0x494b5348u;  // "IKSH"

// One rank's tail block as gathered: the stats record, the plan, then its
// FK-error histogram.
struct IkTailBlock {
  ik_shard_tail t;
  IkPlanHdr plan;
  uint32_t hist[IK_FKHIST_BINS];
};

// One RCCL communicator of a context (ik_comm_init) and the state of the
// chunked in-place all-gathers of the sharded solves (ik_shard.hip), grow-only
// like the scratch.
struct IkComm {
  void *comm = nullptr;  // ncclComm_t (a non-null sentinel for a loopback communicator)
  bool loopback = false;  // ik_comm_init_loopback (test-only): no RCCL, see ik_shard.hip
  int nranks = 0, rank = -1;
  int chunks_req = 0;    // ik_comm_set_chunks (0 = automatic)
  int last_chunks = 0;   // all-gathers of the last sharded call (its plan's chunks)
  int last_req = 0;      // the chunk count that plan was made with (ik_comm_info)
  bool last_hist = false;  // the last sharded call gathered FK-error histograms
  hipStream_t cs = nullptr;  // the gathers' stream
  void *stage = nullptr;     // the ragged last chunk's rows (all regions)
  size_t stage_bytes = 0;
  IkTailBlock *tail_send = nullptr;  // device: this rank's tail block
  IkTailBlock *tail_recv = nullptr;  // device: every rank's
  IkTailBlock *h_tails = nullptr;    // pinned: every rank's
  int tails_n = 0;
  ikhip::DevStats *d_cstats = nullptr;  // one stats block per chunk
  hipEvent_t ev_solved[IK_MAX_GATHER_CHUNKS] = {};  // chunk k's rows written (solve stream)
  hipEvent_t ev_gs[IK_MAX_GATHER_CHUNKS] = {}, ev_ge[IK_MAX_GATHER_CHUNKS] = {};  // gather k
  hipEvent_t ev_done = nullptr;  // the call's last gather / copy on cs
  // Bounded waits (ik_shard.hip comm_wait): every host wait on the collective
  // polls the communicator's async error against this deadline and aborts the
  // communicator when it passes, so a dead or stuck peer ends in IK_E_RCCL
  // instead of a hang.  0 = IKHIP_RCCL_TIMEOUT_S, else 120 s.
  double timeout_s = 0.0;
  bool broken = false;   // aborted (deadline, async error, mid-call failure): calls refuse
  std::string why;       // ... and why
  hipEvent_t ev_end = nullptr;  // the last sharded call's end on its solve stream
  bool ev_end_set = false;
  // ik_comm_loopback_stall (test-only): the loopback all-gathers spin on this
  // pinned flag until the deadline's abort sets it (or their own 30 s cap)
  int *stall_flag = nullptr;
  bool stall = false;
};

// The chunked host-pointer pipeline (ik_pipe.cpp): copy streams, per-chunk
// events and stats blocks, device staging; created on first use.
constexpr int kPipeMaxChunks = 8;
struct IkPipe {
  hipStream_t s_in = nullptr, s_out = nullptr;
  hipEvent_t ev_in[kPipeMaxChunks] = {}, ev_done[kPipeMaxChunks] = {}, ev_out = nullptr;
  ikhip::DevStats *d_stats = nullptr;  // kPipeMaxChunks blocks
  ikhip::DevStats *h_stats = nullptr;  // pinned copies
  void *buf = nullptr;
  size_t buf_bytes = 0;
};

struct ik_ctx {
  int device = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  ikhip::DevStats *d_stats = nullptr;
  ikhip::DevStats *h_stats = nullptr;  // pinned
  void *scratch = nullptr;
  size_t scratch_bytes = 0;
  ikhip::RobotDev robot;
  // the robot's joint limits (ik_set_joint_limits): host state, handed to the refine
  // kernels by value; ik_set_robot leaves them.  A fresh context: every joint free.
  ikhip::JointLimits jlim = {{-HUGE_VAL, -HUGE_VAL, -HUGE_VAL, -HUGE_VAL},
                             {HUGE_VAL, HUGE_VAL, HUGE_VAL, HUGE_VAL}, 0u};
  bool ann_loaded = false;
  ikhip::AnnModelDev ann;
  void *ann_buf = nullptr;
  const void *ann_wx[ikhip::kAnnMaxLayers] = {};  // bf16x6 weight operand of each layer
  const void *ann_wh[ikhip::kAnnMaxLayers] = {};  // fp16x3 weight operand of each layer
  float ann_hinv[ikhip::kAnnMaxLayers] = {};      // fp16x3: 2^-(weight pre-scale exponent)
  int ann_mode = IK_ANN_FP32;
  // a model outside the fused kernel's caps runs layer at a time (ik_ann_big.hip)
  bool ann_big = false;
  ikhip::AnnBigModel ann_bigm;  // its layers (pointers into ann_buf)
  void *ann_act = nullptr;      // its activation buffers, grow-only
  size_t ann_act_bytes = 0;
  // training state (ik_ann_train_begin .. ik_ann_train_end), apart from the loaded model
  ikhip::TrainDev *train = nullptr;
  int fabrik_variant = 1;
  int fabrik_bpc = 0;   // IKHIP_FABRIK_BPC: iteration-kernel blocks per CU (0 = size rule)
  int fabrik_core = 2;  // IKHIP_FABRIK_CORE: 2 core + reuse, 1 sqrt_core / div_core, 0 general
  ikhip::KTimer kt;
  unsigned long long *dbg = nullptr;     // diagnostic stamp buffer (ik_ctx_set_debug)
  ikhip::FabOrderDev *fab_ord = nullptr;  // FABRIK work-order cost table (learned per robot)
  unsigned int *fab_priors = nullptr;     // device copies of the built-in tables (ik_fabrik_prior.h)
  int fab_prior = -1;  // the built-in table fab_ord holds untouched (index), -1 learned / empty
  ikhip::RobotConstDev *rconst = nullptr;  // FABRIK seed-pose constants of the robot
  IkComm comm;
  IkPipe pipe;
  hipStream_t last_stream = nullptr;  // the stream the last solve was enqueued on
  hipEvent_t call_done = nullptr;     // recorded on last_stream at the end of every call
  bool call_done_set = false;
  bool last_sharded = false;  // the last call's stats are in comm.h_tails
  // the gathered tails of the last sharded call (for IK_F_ASYNC + ik_stats_fetch)
  int64_t last_n = 0;
  bool last_piped = false;  // the last call was a chunked host pipeline: its stats are piped_stats
  ik_stats piped_stats = {};
};

namespace ikapi {

int fail(int code, const std::string &msg);

#define IK_HIP(call)                                                                 \
  do {                                                                               \
    hipError_t e_ = (call);                                                          \
    if (e_ != hipSuccess)                                                            \
      return ::ikapi::fail(IK_E_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
  } while (0)

// One enqueueing call: per-kernel HIP-event timing of it (ik_ctx_set_timing),
// and the context's one sequence of device work -- on entry the call's stream
// waits for the previous call's end event when that call ran on another stream;
// on exit the call records its own.
struct KtScope {
  explicit KtScope(ik_ctx *c);
  ~KtScope();
  ik_ctx *c_;
};

// One call's regions of the context's scratch, in the order they are described,
// each on a 256-byte boundary (the kernels store double2 / float4).  Describe
// the regions, reserve() -- the scratch may be reallocated until then -- take
// the device pointers with at(), launch, flush().  Host pointers (no
// IK_F_DEVICE): inputs and present outputs are staged, copied in by reserve()
// and out by flush(), in order.  Device pointers: at() is the caller's own.
// Every copy is asynchronous on the context's stream and nothing here waits
// (finish() does).
class Stage {
 public:
  static size_t up(size_t b) { return (b + 255) & ~(size_t)255; }
  // The layout alone: add a region, get its offset, know the total.
  struct Carve {
    size_t total = 0;
    size_t add(size_t bytes) {
      const size_t at = total;
      total += up(bytes);
      return at;
    }
  };

  Stage(ik_ctx *c, int flags) : c_(c), dev_(flags & IK_F_DEVICE) {}
  // Each returns the region's handle for at().
  int work(size_t bytes) { return add(kWork, nullptr, bytes); }  // device-only, both modes
  // host memory in both modes (the call completes before it returns)
  int table(const void *host, size_t bytes) { return add(kTable, host, bytes); }
  int in(const void *p, size_t bytes) { return add(kIn, p, bytes); }
  // p null: an absent output -- no scratch, a null device pointer, no copy
  int out(void *p, size_t bytes) { return add(kOut, p, bytes); }
  int reserve();  // grows the scratch (once), then queues the host -> device copies
  int flush();    // after the kernels: queues the device -> host copies
  template <class T>
  T *at(int r) const {
    return static_cast<T *>(r_[r].dev);
  }

 private:
  enum Kind { kWork, kTable, kIn, kOut };
  struct Region {
    Kind kind;
    void *user;  // the caller's pointer
    size_t bytes, off;
    bool staged;  // lives in the scratch at `off`
    void *dev;
  };
  static constexpr int kMax = 8;  // (ik_chain_pose_solve)
  int add(Kind kind, const void *user, size_t bytes);
  ik_ctx *c_;
  bool dev_;
  Carve cv_;
  int n_ = 0;
  Region r_[kMax];
};

int ensure_scratch(ik_ctx *c, size_t bytes);
int set_dev(ik_ctx *c);
// The refusals every enqueueing call shares: IK_F_ASYNC needs IK_F_DEVICE, and a
// device `ang` (null: the call has none) is stored 16 bytes at a time.
int check_flags(const char *who, int flags, const void *ang = nullptr);
// What ik_refine, ik_ann_solve_refined and ik_chain_solve refuse alike (ik_api.cpp): a
// NULL context, n < 0, missing arrays with n > 0, max_iter < 0, a NaN tol, a damping
// that is not finite and > 0, then check_flags (ang null: no alignment demanded).
int refine_args(const char *who, ik_ctx *c, int64_t n, bool arrays, double tol, int32_t max_iter,
                double damping, const double *ang, int flags);
void stats_from_dev(const ikhip::DevStats &d, ik_stats *s);
int finish(ik_ctx *c, int flags, ik_stats *stats);
// Device pointers only, on the context's stream: stats reset + the solve's kernels.
// work: fabrik_scratch_bytes(n) of device memory.
// S: the stats block (null: the context's).
int fabrik_launch(ik_ctx *c, const double *dp, int64_t n, double tol, int max_iter, double *da,
                  int32_t *di, double *dj, double *dfe, bool limits, void *work,
                  ikhip::DevStats *S = nullptr);
int ann_launch(ik_ctx *c, const double *dp, int64_t n, float *da, double *de, bool limits,
               ikhip::DevStats *S = nullptr);
// The FABRIK work order of a fresh table (ik_api.cpp): the built-in prior for
// (tol, max_iter) when the robot is SixDOFRobot's chain, else empty.
int seed_order(ik_ctx *c, double tol, int max_iter);
// FABRIK host-pointer solves whose arrays are all pinned (ik_host_alloc) and large enough:
// chunked H2D / solve / D2H on three streams (ik_pipe.cpp).
bool pipeline_wanted(ik_ctx *c, int64_t n, std::initializer_list<const void *> ptrs);
int fabrik_host_pipeline(ik_ctx *c, const double *pts, int64_t n, double tol, int max_iter,
                         double *ang, int32_t *iters, double *joints, double *fk_err, int flags,
                         ik_stats *stats);
void pipe_release(ik_ctx *c);
// Frees the context's training state, if any (ik_train_api.cpp).
void train_release(ik_ctx *c);
// The batch stats of the last sharded call, from the gathered tails (waits).
int sharded_stats(ik_ctx *c, ik_stats *stats);
// Releases the communicator; false when aborted work has not drained (its
// buffers are then left to the process's end).
bool comm_release(ik_ctx *c);
// Waits for `ev` with the communicator's deadline and async-error polling when
// the context holds a live communicator (else a plain hipEventSynchronize).
int comm_wait(ik_ctx *c, hipEvent_t ev, const char *what);

}  // namespace ikapi
