// ik_fabrik.hip -- batched FABRIK inverse kinematics for gfx950.
//
// Restates, one goal point per lane in float64, the reference's
//   FabrikInverseKinematics.ikine   kinematics/inverse.py:115-139
//   Fabrik.calculate / __backward / __forward   kinematics/fabrik.py:19-67
//   __get_angles                    kinematics/inverse.py:54-112
// with the same operation order, so iteration counts are bit-exact.  This unit
// holds the iteration kernels and their launch; the iteration's arithmetic is
// ik_fabrik_step.h, the angles step's ik_fabrik_angles.h, the work order's
// kernels ik_fabrik_order.hip and Fabrik.calculate on its own ik_fabrik_calc.hip.
//
// Two pipelines (DESIGN.md "FABRIK"):
//  * fused (default): classify + scatter (the hard-first work order, 6 bytes
//    per point) -> iter_kernel: persistent; each wave prepares batches of seed
//    poses into its LDS batch, refills the lanes whose points converged from it
//    (so a wave does not wait for its slowest lane), parks finished lanes in an
//    LDS ring and runs the angles step + FK round trip + batch stats on them in
//    batches -> fold (the samples into the cost table).  Seed poses and final
//    joints never touch HBM.
//  * simple: everything in one kernel, one point per lane, no refill.
// Per point the state is 4 joints + goal (15 doubles) held in VGPRs.
#include <algorithm>
#include <cmath>

#include "ik_arith.h"
#include "ik_fabrik.h"
#include "ik_fabrik_angles.h"
#include "ik_fabrik_args.h"
#include "ik_fabrik_plan.h"
#include "ik_fabrik_step.h"
#include "ik_fk_chain.h"
#include "ik_launch.h"
#include "ik_stats.h"

namespace ikhip {

__device__ __forceinline__ void store_joints(double *dst, int64_t i, const d3 J[4]) {
  double *p = dst + 12 * i;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    p[3 * k] = J[k].x;
    p[3 * k + 1] = J[k].y;
    p[3 * k + 2] = J[k].z;
  }
}

// Diagnostic counters of the iteration kernel (-DIKHIP_DIAG, libikhip_diag.so,
// tools/fabrik_diag.py): per wave, summed into dbg[0..7], and per wave w at
// dbg[64 + 4w ..]: s_memrealtime (100 MHz) at start, when the queue ran dry
// for it and at the end, and the steps it ran after the queue ran dry.
enum { kDiagLoops, kDiagSteps, kDiagLaneSteps, kDiagRefills, kDiagGrabs, kDiagFallbacks,
       kDiagWaves, kDiagFlushes, kDiagFlushTicks, kDiagPrepTicks, kDiagRefillTicks,
       kDiagParkTicks, kDiagStageTicks, kDiagCount };
// per-wave record (kDiagWords): the counters above, then s_memrealtime stamps
enum { kDiagTStart = kDiagCount, kDiagTDry, kDiagTLast, kDiagStepsDry, kDiagTDrain, kDiagTEnd,
       kDiagTRefill, kDiagTSub, kDiagDrainN, kDiagTDrain2, kDiagHwId, kDiagWords = 24 };
#ifdef IKHIP_DIAG
constexpr int kDiagWaveMax = 4096;  // = (kFabrikDebugWords - 64) / kDiagWords (24)
#endif

// Phase marks for the instruction census (tools/isa_phases.py): an analysis build
// with -DIKHIP_PHASE_MARKS puts an assembly comment at each phase boundary of the
// iteration kernel; the production build has none.
#ifdef IKHIP_PHASE_MARKS
#define IKHIP_MARK(s) asm volatile(";@phase " s)
#else
#define IKHIP_MARK(s) ((void)0)
#endif

static int env_int(const char *name, int dflt) {
  const char *v = getenv(name);
  return (v && *v) ? atoi(v) : dflt;
}

// A lane's sums of the batch stats over the points it committed (commit_point).
struct LaneAcc {
  unsigned long long sum_it = 0, capped = 0;
  int max_it = 0;
  double fk_max = 0.0, fk_sum = 0.0;
};

// The robot constants' pointer made opaque to the compiler: loads through it are
// issued where they are used (s_load, scalar cache) instead of hoisted out of the
// persistent loop into SGPRs, where the seed and angles steps' ~100 constants
// spilled and the iteration paid for their reloads (v_readlane) every step.
__device__ __forceinline__ RcConst opaque_rc(const RobotConstDev *p) {
  asm volatile("" : "+s"(p));
  return (RcConst)p;
}

__device__ __forceinline__ bool outside_rc(RcConst k, d3 g) {
  const double lim[6] = {k->lim[0], k->lim[1], k->lim[2], k->lim[3], k->lim[4], k->lim[5]};
  return outside(lim, g.x, g.y, g.z);
}

// What the call reports about one finished point once its angles are known:
// angles, iterations, joints, the FK round trip (cli.py:54-61) and the per-lane
// sums of the batch stats.
__device__ __forceinline__ void commit_point(const FabArgs &a, int64_t i, const d3 J[4], d3 g,
                                             int it, int st, const double th[4],
                                             const double cs[4], const double sn[4],
                                             LaneAcc &acc) {
  if (st != IK_OK) record_error(a.S, i, st);
  double2 *o = reinterpret_cast<double2 *>(a.ang + 4 * i);
  o[0] = make_double2(th[0], th[1]);
  o[1] = make_double2(th[2], th[3]);
  if (a.iters) a.iters[i] = it;
  if (a.joints) store_joints(a.joints, i, J);
  acc.sum_it += (unsigned long long)it;
  acc.capped += (it >= a.max_iter) ? 1ull : 0ull;
  acc.max_it = max(acc.max_it, it);
  if (a.fk_err) {
    double e = __builtin_nan("");
    IKHIP_MARK("commit.fk");
    if (st == IK_OK) {
      const RcConst k = opaque_rc(a.rc);
      double jc[16];
#pragma unroll
      for (int e2 = 0; e2 < 16; ++e2) jc[e2] = k->jc[e2];
      // (the angles' own range, forward.py:23-25: always within 2 pi here)
      bool ok = !k->alpha_bad;
#pragma unroll
      for (int e2 = 0; e2 < 4; ++e2) ok = ok && angle_ok(th[e2]);
      e = fk_error_cs(jc, cs, sn, ok, g.x, g.y, g.z);
    }
    IKHIP_MARK("commit.fk_end");
    a.fk_err[i] = e;
    if (e == e) {
      acc.fk_max = fmax(acc.fk_max, e);
      acc.fk_sum += e;
    }
  }
}

// The angles step of one finished point (inverse.py:136 __get_angles): the core
// sequences (get_angles_core); a lane outside their domains is flagged (redo)
// and the whole wave then runs the general get_angles for the flagged lanes in
// a pass of its own, so the general code's registers are never live beside the
// fast path's.  has: the lane holds a point; st: its status so far.
template <class Joints>
__device__ __forceinline__ void angles_step(bool has, Joints joints, int &st, double th[4],
                                            double cs[4], double sn[4]) {
#pragma unroll
  for (int k = 0; k < 4; ++k) th[k] = cs[k] = sn[k] = __builtin_nan("");
  bool redo = false, fast = false;
  if (has && st == IK_OK) {
    d3 J[4];
    joints(J);
    int sf = IK_OK;
    fast = get_angles_core(J, th, sf, cs, sn);
    redo = !fast;
    if (fast) st = sf;
  }
  IKHIP_MARK("angles.general");
  if (__any(redo)) {  // wave-uniform and rare: coincident joints, zero divisors, x = 0 or y = 0
    if (redo) {
      d3 J[4];
      joints(J);
      get_angles(J, th, st);
#pragma unroll
      for (int k = 0; k < 4; ++k) sincos_fk(th[k], &sn[k], &cs[k]);
    }
  }
  // theta_1 (inverse.py:60) last: kept out of the fast pass, whose registers
  // then fit beside the general pass's without spilling
  IKHIP_MARK("angles.atan2");
  if (fast) {
    d3 J[4];
    joints(J);
    th[0] = atan2_fast(J[3].y, J[3].x);
  }
  IKHIP_MARK("angles.end");
}

// ------------------------------------------------------------- simple ----
// One point per lane, no refill: the test variant (IKHIP_FABRIK_VARIANT=0) and
// the solves whose loop runs no iteration at all (max_iter 0, tol >= 1) or whose
// robot FK rejects (its own DH angles out of range: every seed raises).
__global__ __launch_bounds__(256) void fabrik_simple_kernel(FabArgs a) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  LaneAcc acc;
  d3 g = {0.0, 0.0, 0.0}, J[4] = {};
  int st = IK_OK, it = 0;
  if (i < a.n) {
    g = {a.pts[3 * i], a.pts[3 * i + 1], a.pts[3 * i + 2]};
    if (a.check_limits && outside(a.r.lim, g.x, g.y, g.z))
      atomicMin(&a.S->first_oob, (unsigned long long)i);
    // Seed pose, inverse.py:123-130: FK of [atan2(y, x), thetas[1:]] (the
    // reference writes theta_1 into dh_matrix[0][0] and runs fkine on that row), in
    // closed form from the per-robot constants (seed_closed, ik_fk_chain.h; r05 and
    // before: seed_chain, the DH chain's own products).
    st = seed_closed(a.rc, g, J);
    double se = 1.0, ge = 1.0;
    if (st == IK_OK) {
      while (((se > a.tol2) || (ge > a.tol2)) && (a.max_iter > it)) {
        fabrik_step4(J[0], J[1], J[2], J[3], g, a.r.links, se, ge, st);
        ++it;
        if (st != IK_OK) break;
      }
    }
  }
  double th[4], cs[4], sn[4];
  angles_step(i < a.n, [&](d3 *o) {
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = J[k];
  }, st, th, cs, sn);
  if (i < a.n) commit_point(a, i, J, g, it, st, th, cs, sn, acc);
  block_iter_stats_acc(a.S, acc.sum_it, acc.capped, acc.max_it);
  if (a.fk_err) wave_fk_stats(a.S, acc.fk_max, acc.fk_sum);
}

// The whole FABRIK solve of one goal in the general arithmetic (the simple
// kernel's loop: fabrik.py:44-67 from the seed pose, inverse.py:123-133): the
// iteration kernel's retire step re-solves the rare lanes whose core sequences
// left their domain (kStRedo) with it.  (The simple kernel keeps its own copy of
// the loop: with a call of this function the compiler emits other code for it.)
__device__ __forceinline__ void solve_general(const FabArgs &a, d3 g, d3 J[4], int &it,
                                              int &st) {
  st = seed_closed(a.rc, g, J);
  it = 0;
  double se = 1.0, ge = 1.0;
  if (st != IK_OK) return;
  while (((se > a.tol2) || (ge > a.tol2)) && (a.max_iter > it)) {
    fabrik_step4(J[0], J[1], J[2], J[3], g, a.r.links, se, ge, st);
    ++it;
    if (st != IK_OK) break;
  }
}
// A lane of the iteration kernel whose core sequences left their domain
// (coincident joints, non-finite or extreme coordinates: sqrt_core / div_core
// would not give the general sequences' bits) stops with this status; the retire
// step re-solves its goal with solve_general (r06: no copy of the pre-step state
// is kept for an in-loop redo).
constexpr int kStRedo = 0x40;

// Persistent iteration with per-lane refill, seed and angles in batches (the work
// order's launch 3, between scatter and fold: ik_fabrik_order.hip).
//
// A lane whose point converged is refilled from the wave's batch of prepared
// points: a wave grabs a.chunk queue positions at once and each lane prepares one
// of them -- the goal, the limits check and the seed pose (inverse.py:123-130) --
// into the wave's LDS batch, at full SIMD width; a refill then hands entries to
// the free lanes (LDS reads), with no memory round trip.
// A finished lane parks its final joints in the wave's LDS ring at the next
// refill; when the ring would overflow, and at the end, the whole wave runs the
// angles step on it, one entry per lane (finish_point).  So the seed pose and
// the joints never travel through HBM, and neither step runs at the width of
// the handful of lanes that finish together.
// A parked point is one 144-byte record per slot, written and read as nine
// 16-byte words (ds_write_b128 / ds_read_b128): the joints, the goal (for the FK
// round trip, not read from HBM again) and {index, iterations, status}.  The
// 36-dword slot stride puts 16 lanes' words on 64 distinct banks.
struct RetireRing {
  double2 w[64][9];
};

__device__ __forceinline__ void ring_put(RetireRing &R, int s, const d3 &J0, const d3 &J1,
                                         const d3 &J2, const d3 &J3, const d3 &g, int64_t idx,
                                         int it, int st) {
  double2 *w = R.w[s];
  w[0] = {J0.x, J0.y};
  w[1] = {J0.z, J1.x};
  w[2] = {J1.y, J1.z};
  w[3] = {J2.x, J2.y};
  w[4] = {J2.z, J3.x};
  w[5] = {J3.y, J3.z};
  w[6] = {g.x, g.y};
  w[7] = {g.z, 0.0};
  w[8] = {__longlong_as_double(idx),
          __longlong_as_double((long long)(((uint64_t)(uint32_t)st << 32) | (uint32_t)it))};
}

__device__ __forceinline__ void ring_joints(const RetireRing &R, int s, d3 *J) {
  const double2 *w = R.w[s];
  const double2 w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3], w4 = w[4], w5 = w[5];
  J[0] = {w0.x, w0.y, w1.x};
  J[1] = {w1.y, w2.x, w2.y};
  J[2] = {w3.x, w3.y, w4.x};
  J[3] = {w4.y, w5.x, w5.y};
}

// The angles step over the ring's first cnt entries (the whole wave calls it).
// ORD: 1 in kOrdSample points records (cell, iterations) for the cost table.
// IKHIP_FAB_PRIO: the angles step and the seed preparation run at a raised wave
// priority.  Two waves share a SIMD and, at equal priority, the older one's VALU
// wins every issue arbitration (MI355X_MICROARCH.md, "Two waves per SIMD"): a
// younger wave's angles step -- long dependent chains, few instructions ready at
// a time -- then gets only the slots its iterating partner leaves and took 10-50 us
// instead of 2.5 for one wave in ten at the end of the launch.  Raised, it issues
// whenever it has an instruction ready and the partner's issue-bound iteration
// fills the rest.
#ifndef IKHIP_FAB_PRIO
#define IKHIP_FAB_PRIO 2
#endif
__device__ __forceinline__ void prio_raise() {
  if (IKHIP_FAB_PRIO) __builtin_amdgcn_s_setprio(IKHIP_FAB_PRIO);
}
__device__ __forceinline__ void prio_drop() {
  if (IKHIP_FAB_PRIO) __builtin_amdgcn_s_setprio(0);
}

template <bool ORD>
__device__ __forceinline__ void ring_flush(const FabArgs &a, RetireRing &R, int cnt, int lane,
                                           LaneAcc &acc) {
  prio_raise();
  IKHIP_MARK("flush.angles");
  __builtin_amdgcn_wave_barrier();
  const bool has = lane < cnt;
  // the joints from the ring each time they are needed (LDS reads are cheap; the
  // barrier keeps the compiler from holding them in registers across the step)
  auto joints = [&](d3 *J) {
    asm volatile("" ::: "memory");
    ring_joints(R, lane, J);
  };
  double2 meta = R.w[lane][8];
  uint64_t itst = (uint64_t)__double_as_longlong(meta.y);
  int st = has ? (int)(itst >> 32) : IK_OK;
  if (__builtin_expect(__any(has && st == kStRedo), 0)) {  // wave-uniform, rare
    if (has && st == kStRedo) {
      const double2 g01 = R.w[lane][6], g2 = R.w[lane][7];
      d3 J[4];
      int it2;
      solve_general(a, {g01.x, g01.y, g2.x}, J, it2, st);
      ring_put(R, lane, J[0], J[1], J[2], J[3], {g01.x, g01.y, g2.x},
               __double_as_longlong(meta.x), it2, st);
      itst = ((uint64_t)(uint32_t)st << 32) | (uint32_t)it2;
    }
    __builtin_amdgcn_wave_barrier();
  }
  double th[4], cs[4], sn[4];
  angles_step(has, joints, st, th, cs, sn);
  IKHIP_MARK("flush.commit");
  if (has) {
    d3 J[4];
    joints(J);
    const int64_t i = __double_as_longlong(meta.x);
    const int it = (int)(uint32_t)itst;
    const double2 g01 = R.w[lane][6], g2 = R.w[lane][7];
    commit_point(a, i, J, {g01.x, g01.y, g2.x}, it, st, th, cs, sn, acc);
    if constexpr (ORD) {
      if (i % kOrdSample == 0 && i / kOrdSample < kOrdMaxSample) {
        const uint32_t lo = (uint32_t)(it < 0xffff ? it : 0xffff);
        a.ord->sample[i / kOrdSample] = ((uint32_t)(a.cell[i] & (kOrdCells - 1)) << 16) | lo;
      }
    }
  }
  IKHIP_MARK("flush.end");
  __builtin_amdgcn_wave_barrier();
  prio_drop();
}


// ORD: the queue is a.perm (ik_fabrik_order.hip), else point order.  CORE: 0
// general sqrt / division, 1 sqrt_core / div_core, 2 the same with the repeated
// distances taken once and the loop condition from the band (fabrik_step4_lazy;
// needs L0 == L1 and L2 == L3).
// Every solve reaching this kernel runs at least one iteration (the host sends
// the others to fabrik_simple_kernel), so the seed's last joint is never needed.
#ifndef IKHIP_FAB_REFILL  // free lanes that trigger a refill (r05: 12 against 6 / 8 / 16 / 20 / 24 / 32; 12 since the dry waves' raised priority; r06 on the 142-VALU loop: 8 +1.5-4 %, 16 even-+1.4 %)
#define IKHIP_FAB_REFILL 12
#endif
#ifndef IKHIP_ITER_WAVES
#define IKHIP_ITER_WAVES 2
#endif
// The refill (park, stage, hand-out) runs at raised wave priority, like the seed and
// angles steps: its dependent chains issue when ready instead of in the partner's
// leftover slots.  r04, same box: iteration kernel -1.7 % at tol 1e-3, -1.3 % at 1e-5
// (rocprof windows, 3 / 2 runs each), -1.0 / -1.3 % per bench step in another lease.
// (r04: taking the seed's carried quotient in the prepare step instead of at the
// hand-out measured slower, profiles/r04/ab/fabrik_refill_prio_prep_carry.txt; r06
// takes it there as part of a bundle that measured faster, DESIGN_HISTORY.md.)
constexpr int kIterWaves = IKHIP_ITER_WAVES;  // waves per SIMD = blocks per CU
template <int REFILL_MIN, bool ORD, int CORE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(kIterWaves, kIterWaves))) void
fabrik_iter_kernel(FabArgs a) {
  __shared__ RetireRing rings[4];
  const int lane = threadIdx.x & 63;
  RetireRing &R = rings[threadIdx.x >> 6];
  const unsigned long long lt_mask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
  // the loop condition's operands held in VGPRs: as wave-uniform values they
  // compete for the SGPRs the nested exec masks need, and the compiler then
  // re-read tol2 from the kernel arguments (s_load + wait) every iteration
  double tol2 = a.tol2;
  int max_iter = a.max_iter;
  asm volatile("" : "+v"(tol2), "+v"(max_iter));
  // the goal error's threshold as an opaque second copy: with one value on both
  // compares, (se > t) || (ge > t) becomes max(se, ge) > t, three v_max_f64 (two
  // canonicalizing) and a compare instead of two compares
  double tol2g = tol2;
  asm volatile("" : "+v"(tol2g));
  double qmax = a.qmax;  // (CORE 2: fabrik_step4_lazy's domain test, also in a VGPR)
  asm volatile("" : "+v"(qmax));
  double L[4] = {a.r.links[0], a.r.links[1], a.r.links[2], a.r.links[3]};

  // prepared points: the batch's entry j in slot j of the wave's LDS batch
  // (wave-uniform count / cursor); a refilled lane reads its entry from there
  struct PrepBatch {  // per entry seven 16-byte words: seed joints 0..2, goal, {meta, cq}
    double2 w[64][7];
  };
  // an entry's meta word: the point index, and (CORE 2, bit 62) whether the point
  // goes straight to the retire step's general re-solve: the seed's carried
  // radicand outside the core domain, or a start / goal past the launch's error
  // band (|J0|_1 + |goal|_1 > band_n1, or not finite) -- the carry itself
  // (reuse_carry) and the band test are taken at full width in the preparation,
  // not per refill (r06)
  constexpr uint64_t kMetaRedo = 1ull << 62;
  __shared__ PrepBatch batches[4];
  PrepBatch &PB = batches[threadIdx.x >> 6];
  int pcount = 0, pptr = 0;
  // the next batch, fetched in stages while the current one is handed out (so
  // that no stage waits for memory): 0 none, 1 queue grab issued (na), 2 its
  // permutation entries loaded (nperm), 3 its goals loaded (ng, ni); -1 the queue is dry
  int nstage = 0, ncount = 0;
  int64_t nbase = 0;
  // the queue head this wave grabs from (its block's, blockIdx % kQueueHeads,
  // until that one runs dry; then the next one its block has not seen dry)
  __shared__ unsigned int dry_heads;  // the heads this block found dry
  if (threadIdx.x == 0) dry_heads = 0;
  __syncthreads();
  int head = (int)(blockIdx.x % kQueueHeads);
  unsigned long long na = 0;
  // (nperm as loaded, 32 bits, widened by the stage that uses it, and the goal as
  // three separate loads: each lands in the register the preparation reads, so no
  // copy waits for a load right after its issue)
  int32_t nperm = 0;
  int64_t ni = 0;
  d3 ng = {0, 0, 0};
  bool dry = false;   // the queue and the batch are exhausted
  int rcnt = 0;       // entries in the retire ring
  LaneAcc acc;

  bool active = false, pending = false;  // solving / finished but not yet parked
  int64_t out = 0;                       // the lane's point index
  // J3: the effector; CORE 2 keeps it only from a fallback iteration (the fast
  // step leaves it to the carry: effector() below)
  d3 J0 = {0, 0, 0}, J1 = J0, J2 = J0, J3 = J0, g = J0;
  bool cont = true;  // the reference's loop condition after the lane's last iteration
  int st = IK_OK;
  // the lane's iteration count as step - max_iter (mod 2^32): the increment's
  // carry is the cap (fabrik.py:57 iteration < max_iter), folded into cont, so
  // the loop's run test needs no compare of its own (r06)
  uint32_t kst = 0;
  auto steps = [&]() -> int { return (int)(kst + (uint32_t)max_iter); };
  double cq = 0.0;  // CORE == 2: the carried quotient and offset
  d3 cd = J0;
  bool cbad = false;  // CORE == 2: the taken entry goes to the retire step's re-solve
  // the effector F3 = get_point_between(F2, goal, L3): CORE 2 from the carry (cq,
  // cd = goal - F2; a lane whose radicands left the core domain is re-solved at
  // retire, kStRedo), else the step's J3
  auto effector = [&]() -> d3 {
    if constexpr (CORE == 2) return {J2.x + (cq * cd.x), J2.y + (cq * cd.y), J2.z + (cq * cd.z)};
    return J3;
  };

#ifdef IKHIP_DIAG
  // counters and stamps live in LDS (lane 0 writes), so that the diagnostic
  // build keeps the production kernel's registers and occupancy
  __shared__ unsigned long long dgs[4][kDiagWords];
  unsigned long long *dg = dgs[threadIdx.x >> 6];
  if (lane < kDiagWords) dg[lane] = 0;
  __builtin_amdgcn_wave_barrier();
  if (lane == 0) dg[kDiagTStart] = __builtin_amdgcn_s_memrealtime();
  // where the wave runs: XCC_ID (hwreg 20) << 32 | HW_ID (hwreg 4: wave 3:0, SIMD 5:4, CU 11:8, SE 14:13)
  if (lane == 0)
    dg[kDiagHwId] = ((unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 20) << 32) |
                    (unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 4);
#define IKHIP_DG(k, v) \
  do {                 \
    if (lane == 0) dg[k] += (v); \
  } while (0)
#define IKHIP_DT(k) \
  do {              \
    if (lane == 0) dg[k] = __builtin_amdgcn_s_memrealtime(); \
  } while (0)
#define IKHIP_DT_ACC(k, k0) \
  do {                      \
    if (lane == 0) dg[k] += __builtin_amdgcn_s_memrealtime() - dg[k0]; \
  } while (0)
#else
#define IKHIP_DG(k, v) ((void)0)
#define IKHIP_DT(k) ((void)0)
#define IKHIP_DT_ACC(k, k0) ((void)0)
#endif
  while (true) {
    const unsigned long long freem = __ballot(!active);
    const int nfree = __popcll(freem);
    if (dry && nfree == 64) break;
    IKHIP_DG(kDiagLoops, 1);
    if (!dry && (nfree >= REFILL_MIN || nfree == 64)) {
      prio_raise();
      IKHIP_MARK("refill.park");
      IKHIP_DG(kDiagRefills, 1);
      IKHIP_DT(kDiagTRefill);  // refill time, less the flushes and preparations in it
      IKHIP_DT(kDiagTSub);
      // park the lanes that finished since the last refill
      const unsigned long long pm = __ballot(pending);
      const int np = __popcll(pm);
      if (np) {
        if (rcnt + np > 64) {
          IKHIP_DG(kDiagFlushes, 1);
          IKHIP_DT_ACC(kDiagParkTicks, kDiagTSub);  // (the park's time excludes the flush)
          IKHIP_DT(kDiagTEnd);  // (scratch slot: the flush's start)
          ring_flush<ORD>(a, R, rcnt, lane, acc);
          prio_raise();  // (the flush dropped it)
          IKHIP_DT_ACC(kDiagFlushTicks, kDiagTEnd);
          IKHIP_DT_ACC(kDiagTRefill, kDiagTEnd);  // (not refill time)
          IKHIP_DT(kDiagTSub);
          rcnt = 0;
        }
        if (pending)
          ring_put(R, rcnt + __popcll(pm & lt_mask), J0, J1, J2, effector(), g, out, steps(), st);
        pending = false;
        rcnt += np;
      }
      IKHIP_DT_ACC(kDiagParkTicks, kDiagTSub);
      IKHIP_DT(kDiagTSub);
      IKHIP_MARK("refill.handout");
      // the next batch's three stages (called below: one per refill ahead of time,
      // or back to back just before a preparation)
      auto stage1 = [&]() {
        if (lane == 0) na = atomicAdd(&a.S->heads[head][0], 1ull);
        nstage = 1;
      };
      auto stage2 = [&]() {
        // the grab's chunk: head h's k-th is the queue's (k * kQueueHeads + h)-th
        // (lane 0's value read into SGPRs: a shuffle would leave the batch's count,
        // cursor and the hand-out divergent in the compiler's eyes)
        const uint64_t na0 =
            ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(na >> 32), 0) << 32) |
            (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)na, 0);
        nbase = ((int64_t)na0 * kQueueHeads + head) * a.chunk;
        if (nbase >= a.n) {  // this head is dry: on to one the block has not seen dry
          if (lane == 0) atomicOr(&dry_heads, 1u << head);
          const unsigned m =
              __builtin_amdgcn_readfirstlane(__hip_atomic_load(&dry_heads, __ATOMIC_RELAXED,
                                                               __HIP_MEMORY_SCOPE_WORKGROUP)) |
              (1u << head);
          if (m == (1u << kQueueHeads) - 1) {
            nstage = -1;
            return;
          }
          int h = head;
          do h = (h + 1) % kQueueHeads;
          while ((m >> h) & 1u);
          head = h;
          nstage = 0;
          return;
        }
        ncount = (int)min((int64_t)a.chunk, a.n - nbase);
        if (lane < ncount) {
          if (ORD) nperm = a.perm[nbase + lane];
        }
        nstage = 2;
      };
      auto stage3 = [&]() {
        if (lane < ncount) {
          const int64_t ip = ORD ? (int64_t)nperm : nbase + lane;
          int64_t iy = 3 * ip + 1, iz = 3 * ip + 2;
          asm volatile("" : "+v"(iy), "+v"(iz));  // (three loads, not a merged x4 + x2)
          ng = {a.pts[3 * ip], a.pts[iy], a.pts[iz]};
          ni = ip;
        }
        nstage = 3;
      };
      // hand prepared points to the free lanes: first what the batch holds, then, if
      // the batch runs out, from the next one.  Straight-line code with one call
      // site per stage: each stage's loads land in the registers the next stage
      // reads, with no merge copies that would wait for them right after issue.
      const bool wasfree = !active;
      const int rank = __popcll(freem & lt_mask);
      const int avail = pcount - pptr;
      const int take1 = min(nfree, avail);
      const bool prep = nfree > avail;  // the batch runs out: prepare the next one
      bool mine = wasfree && rank < take1;
      auto take_entry = [&](int src) {
        const double2 *w = PB.w[src];
        const double2 w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3], w4 = w[4], w5 = w[5];
        J0 = {w0.x, w0.y, w1.x};
        J1 = {w1.y, w2.x, w2.y};
        J2 = {w3.x, w3.y, w4.x};
        g = {w4.y, w5.x, w5.y};
        const double2 w6 = w[6];
        const uint64_t meta = (uint64_t)__double_as_longlong(w6.x);
        out = (int64_t)(meta & (kMetaRedo - 1));
        if constexpr (CORE == 2) {
          // the seed's carry (reuse_carry): cd = goal - J2, exact, as it computes it
          cq = w6.y;
          cd = {g.x - J2.x, g.y - J2.y, g.z - J2.z};
          cbad = (meta & kMetaRedo) != 0;
        }
      };
      // (read before a preparation overwrites the batch)
      if (mine) take_entry(pptr + rank);
      pptr += take1;
      // the next batch's stages: while the batch is down to its last 24 / 16 / 8
      // entries, one per refill (a stage consumes what the one before loaded, so the
      // loads are long done); before a preparation, the stages still missing.  No
      // loop: when stage 2 finds its head dry (back to stage 1 on another), the free
      // lanes stay free, the inner loop returns at once and the next refill goes on.
      // (diagnostic build: before a preparation the stages count as preparation time,
      // as the r04 / r05 breakdowns did, so that staging is the lookahead's cost)
      IKHIP_MARK("refill.stages");
      if (prep) IKHIP_DT(kDiagTDrain);  // (scratch slot: the preparation's start)
      bool more = true;
      if (nstage == 0 && (prep || avail <= 24)) { stage1(); more = prep; }
      if (more && nstage == 1 && (prep || avail <= 16)) { stage2(); more = prep; }
      if (more && nstage == 2 && (prep || avail <= 8)) stage3();
      if (!prep) IKHIP_DT_ACC(kDiagStageTicks, kDiagTSub);
      if (prep && nstage == 3) {
        IKHIP_DG(kDiagGrabs, 1);
        // prepare: limits check and seed pose of the batch, one entry per lane
        pcount = ncount;
        nstage = 0;
        prio_raise();
        IKHIP_MARK("refill.prepare");
        if (lane < pcount) {
          const RcConst k = opaque_rc(a.rc);
          if (a.check_limits && outside_rc(k, ng))
            atomicMin(&a.S->first_oob, (unsigned long long)ni);
          d3 Js[4];
          (void)seed_closed((const RobotConstDev *)k, ng, Js);
          uint64_t meta = (uint64_t)ni;
          double pcq = 0.0;
          if constexpr (CORE == 2) {
            d3 pcd;
            uint32_t pcdom;
            reuse_carry(Js[2], ng, L[3], pcq, pcd, pcdom);
            const bool pbok = fabs(Js[0].x) + fabs(Js[0].y) + fabs(Js[0].z) + fabs(ng.x) +
                                  fabs(ng.y) + fabs(ng.z) <=
                              a.band_n1;
            meta |= (pcdom < kCoreDom && pbok) ? 0ull : kMetaRedo;
          }
          double2 *w = PB.w[lane];
          w[0] = {Js[0].x, Js[0].y};
          w[1] = {Js[0].z, Js[1].x};
          w[2] = {Js[1].y, Js[1].z};
          w[3] = {Js[2].x, Js[2].y};
          w[4] = {Js[2].z, ng.x};
          w[5] = {ng.y, ng.z};
          w[6] = {__longlong_as_double((long long)meta), pcq};
        }
#ifdef IKHIP_DIAG
        // (the seed's loads are consumed before the stamp)
        __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): the batch's LDS writes landed
#endif
        IKHIP_DT_ACC(kDiagPrepTicks, kDiagTDrain);
        IKHIP_DT_ACC(kDiagTRefill, kDiagTDrain);  // (not refill time)
        // the rest of the free lanes from the new batch (a short last chunk may leave
        // some free until the next refill)
        IKHIP_MARK("refill.handout2");
        const int take2 = min(nfree - take1, pcount);
        const bool mine2 = wasfree && rank >= take1 && rank < take1 + take2;
        __builtin_amdgcn_wave_barrier();  // the batch's LDS writes before the reads
        if (mine2) take_entry(rank - take1);
        pptr = take2;
        mine = mine || mine2;
      }
      IKHIP_MARK("refill.start");
      if (mine) {
        st = IK_OK;
        cont = true;  // the loop's initial errors of 1.0 (fabrik.py:53-54) exceed tol
        kst = 0u - (uint32_t)max_iter;
        active = true;
        // (CORE 2: the carry came with the entry, take_entry; an entry the
        // preparation sent to the re-solve -- its carry outside the core domain,
        // or its goal past the band -- stops before its first iteration, for the
        // retire step's solve_general)
        if constexpr (CORE == 2) {
          if (cbad) {
            st = kStRedo;
            cont = false;
          }
        }
      }
      IKHIP_MARK("refill.end");
      dry = nstage < 0 && pptr >= pcount;
      IKHIP_DT_ACC(kDiagRefillTicks, kDiagTRefill);
      // a dry wave's last lanes are the launch's tail: they iterate at priority 1,
      // ahead of a SIMD partner that still hands out its batch (r05, three boxes:
      // iteration kernel -0.7..-1.0 % at tol 1e-3, -0.8..-1.8 % at 1e-5; priority 3,
      // above the partner's refill and angles steps, and refilling at 4 / 8 free
      // lanes once the queue is dry both measured slower: profiles/r05/lease_dry/)
      if (dry) __builtin_amdgcn_s_setprio(1);
      else prio_drop();
    }
    // iterate until a refill is due (REFILL_MIN lanes free) or, once the queue is
    // dry, until every lane has stopped: the refill's scalar state stays out of
    // this loop, so its SGPRs are not reloaded from their spill lanes per iteration
    IKHIP_MARK("loop");
    const int need = __builtin_amdgcn_readfirstlane(dry ? 64 : REFILL_MIN);  // (an SGPR)
    // (r06: the loop's control as uint64 wave masks instead of these lane bools
    // measured worse in the ISA: the masks, updated inside the divergent step,
    // went to VGPRs and took ~25 VALU per iteration; the bools live in SGPR lane
    // masks already, and only ballot(!run) costs a v_cndmask + v_cmp -- also
    // written as exec & ~ballot(run), and with the band flag as a wave mask taken
    // at the refill, which put the wave's exec in VGPRs)
    while (true) {
#ifdef IKHIP_DIAG
    {
      const unsigned long long sm =
          __ballot(active && st == IK_OK && cont);
      IKHIP_DG(kDiagSteps, sm ? 1 : 0);
      IKHIP_DG(kDiagLaneSteps, __popcll(sm));
      if (dry) {  // the queue and the wave's batch are exhausted
        if (lane == 0 && dg[kDiagTDry] == 0) dg[kDiagTDry] = __builtin_amdgcn_s_memrealtime();
        IKHIP_DG(kDiagStepsDry, sm ? 1 : 0);
      }
      if (sm) IKHIP_DT(kDiagTLast);
    }
#endif
    {
      // one divergent region per iteration: lanes that stop here become pending
      // (parked at the next refill) without a branch of their own.  (No st test:
      // every step that sets an error status also clears cont -- the general
      // step's errors give NaN errors, whose comparisons are false, and the core
      // step's kStRedo clears it explicitly.)
      const bool run = active && cont;  // (cont holds the cap: kst)
      pending = pending || (active && !run);
      active = run;
      if (__popcll(__builtin_amdgcn_ballot_w64(!run)) >= need) break;  // (a bool: no VGPR round trip)
      if (run) {
        if constexpr (CORE == 2) {
          // in place: a lane whose radicands leave the core domain stops with
          // kStRedo and the retire step re-solves it in the general arithmetic
          // (solve_general), so no copy of the pre-step state is kept (r06: the
          // wave-wide in-loop redo needed one, 7 register moves per iteration)
          if (!fabrik_step4_lazy(J0, J1, J2, g, L, a.band, tol2, qmax, cont, cq, cd)) {
            st = kStRedo;
            cont = false;
          }
        } else if constexpr (CORE == 1) {
          // wave-uniform fallback: when any lane's radicand leaves sqrt_core's
          // domain (coincident joints, non-finite input) the wave redoes the
          // iteration with the general sqrt / division (and their errors)
          uint32_t dom = 0;
          d3 n1 = J1, n2 = J2, n3 = J3;
          double se, ge;
          fabrik_step4_core(J0, n1, n2, n3, g, L, se, ge, dom);
          if (__all(dom < kCoreDom)) {
            J1 = n1; J2 = n2; J3 = n3;
          } else {
            IKHIP_DG(kDiagFallbacks, 1);
            fabrik_step4(J0, J1, J2, J3, g, L, se, ge, st);
          }
          cont = (se > tol2) || (ge > tol2g);
        } else {
          double se, ge;
          fabrik_step4(J0, J1, J2, J3, g, L, se, ge, st);
          cont = (se > tol2) || (ge > tol2g);
        }
        if (__builtin_add_overflow(kst, 1u, &kst)) cont = false;  // max_iter reached
      }
    }
    }
  }
  // drain: park the last finished lanes, then the angles step on the ring
  IKHIP_MARK("drain");
  IKHIP_DT(kDiagTDrain);
  {
    const unsigned long long pm = __ballot(pending);
    const int np = __popcll(pm);
    IKHIP_DG(kDiagDrainN, rcnt + np);
    if (rcnt + np > 64) {
      ring_flush<ORD>(a, R, rcnt, lane, acc);
      rcnt = 0;
    }
    IKHIP_DT(kDiagTDrain2);
    if (pending)
      ring_put(R, rcnt + __popcll(pm & lt_mask), J0, J1, J2, effector(), g, out, steps(), st);
    rcnt += np;
    IKHIP_DG(kDiagFlushes, 1);
    IKHIP_DT(kDiagTEnd);
    ring_flush<ORD>(a, R, rcnt, lane, acc);
    IKHIP_DT_ACC(kDiagFlushTicks, kDiagTEnd);
  }
#ifdef IKHIP_DIAG
  IKHIP_DT(kDiagTEnd);
  IKHIP_DG(kDiagWaves, 1);
  __builtin_amdgcn_wave_barrier();
  if (a.dbg) {
    const int w = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    if (lane < kDiagCount) atomicAdd(&a.dbg[lane], dg[lane]);
    if (w < kDiagWaveMax && lane < kDiagWords) a.dbg[64 + kDiagWords * w + lane] = dg[lane];
  }
#endif
#undef IKHIP_DG
#undef IKHIP_DT
#undef IKHIP_DT_ACC
  block_iter_stats_acc(a.S, acc.sum_it, acc.capped, acc.max_it);
  if (a.fk_err) wave_fk_stats(a.S, acc.fk_max, acc.fk_sum);
  // (ORD: the cost table is folded by fabrik_fold_kernel, launched next on the
  // same stream: the kernel boundary publishes the sample stores, so no block
  // fences them here -- a release per wave, and later one per block, wrote the
  // XCD's L2 back while the last waves were still draining, r03)
}

static size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

size_t fabrik_scratch_bytes(int64_t n) {
  // work order: perm n int32, cell n uint16
  return up256((size_t)n * 4) + up256((size_t)n * 2) + 1024;
}

template <int REFILL_MIN, bool ORD>
static void launch_iter(int core, unsigned grid, hipStream_t stream, const FabArgs &a) {
  if (core == 2)
    IK_LAUNCH((fabrik_iter_kernel<REFILL_MIN, ORD, 2>), dim3(grid), dim3(256), 0,
                       stream, a);
  else if (core == 1)
    IK_LAUNCH((fabrik_iter_kernel<REFILL_MIN, ORD, 1>), dim3(grid), dim3(256), 0,
                       stream, a);
  else
    IK_LAUNCH((fabrik_iter_kernel<REFILL_MIN, ORD, 0>), dim3(grid), dim3(256), 0,
                       stream, a);
}

void launch_fabrik_ikine(const RobotDev &r, const double *pts, int64_t n, double tol,
                         int max_iter, double *ang, int32_t *iters, double *joints,
                         double *fk_err, bool check_limits, void *scratch, DevStats *S,
                         hipStream_t stream, int variant, int core_req, FabOrderDev *ord,
                         const RobotConstDev *rc, unsigned long long *dbg, int bpc_req,
                         bool prior) {
  if (n <= 0) return;
  // every decision of the launch (ik_fabrik_plan.cpp); the environment is read once
  static const int order_on = env_int("IKHIP_FABRIK_ORDER", 1);
  static const int chunk = env_int("IKHIP_FABRIK_CHUNK", 64);
  FabPlanIn in;
  std::copy(r.dh, r.dh + 16, in.dh);
  std::copy(r.links, r.links + 4, in.links);
  in.n = n;
  in.tol = tol;
  in.max_iter = max_iter;
  in.variant = variant;
  in.core_req = core_req;
  in.bpc_req = bpc_req;
  in.has_table = ord != nullptr;
  in.order_env = order_on;
  in.chunk_env = chunk;
  in.cus = num_cus();
  in.ord_ppt = kOrdPPT;
  in.iter_waves = kIterWaves;
  const FabPlan p = fabrik_plan(in);
  FabArgs a;
  a.r = r;
  a.rc = rc;
  a.dbg = dbg;
  a.pts = pts;
  a.n = n;
  a.tol = tol;
  a.tol2 = p.tol2;
  a.band = p.band;
  a.band_n1 = p.band_n1;
  a.qmax = p.qmax;
  a.max_iter = max_iter;
  a.check_limits = check_limits ? 1 : 0;
  a.ang = ang;
  a.iters = iters;
  a.joints = joints;
  a.fk_err = fk_err;
  a.S = S;
  a.chunk = p.chunk;
  a.perm = nullptr;
  a.cell = nullptr;
  a.ord = ord;
  a.prior_gate = prior ? 1 : 0;
  if (p.simple) {
    kt_begin("fabrik_simple_kernel", stream);
    IK_LAUNCH(fabrik_simple_kernel, dim3(p.grid), dim3(256), 0, stream, a);
    kt_end(stream);
    return;
  }
  if (p.ordered) {
    char *sp = static_cast<char *>(scratch);
    a.perm = reinterpret_cast<int32_t *>(sp);
    sp += up256((size_t)n * 4);
    a.cell = reinterpret_cast<uint16_t *>(sp);
    launch_fabrik_order(a, p.ogrid, stream);
  }
#ifdef IKHIP_DIAG
  if (a.dbg) (void)hipMemsetAsync(a.dbg, 0, kFabrikDebugWords * 8, stream);
#endif
  kt_begin("fabrik_iter_kernel", stream);
  if (p.refill1) {
    if (p.ordered) launch_iter<1, true>(p.core, p.pgrid, stream, a);
    else launch_iter<1, false>(p.core, p.pgrid, stream, a);
  } else {
    if (p.ordered) launch_iter<IKHIP_FAB_REFILL, true>(p.core, p.pgrid, stream, a);
    else launch_iter<IKHIP_FAB_REFILL, false>(p.core, p.pgrid, stream, a);
  }
  kt_end(stream);
  if (p.ordered) launch_fabrik_fold(a, stream);
}

}  // namespace ikhip
