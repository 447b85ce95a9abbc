/*
 * ikhip.h -- C ABI of libikhip.so, the MI355X (gfx950) batched inverse-kinematics
 * engine.  Plain pointers and sizes only; no torch or HIP types in the
 * signatures (streams are passed as void*, a hipStream_t underneath).
 *
 * Each entry point replaces one function of the reference
 * (lstar93/InverseKinematicsANN, file:line below).  The reference is pure
 * Python and has no FFI of its own; the binding a maintainer would add on the
 * reference side is a ctypes stub, shown in INTEGRATION.md.
 *
 * Pointer convention: by default every array argument is a HOST pointer and the
 * call blocks until results are back in host memory.  With IK_F_DEVICE the
 * array arguments are device pointers (e.g. torch tensors' data_ptr()) on the
 * context's device, and with IK_F_ASYNC the call only enqueues work on the
 * context's stream (stats are then read with ik_stats_fetch()).
 *
 * Error convention: every call returns an ik_status.  Per-point failures of the
 * reference (its exceptions) are NOT call failures: they are reported in
 * ik_stats (first_oob / first_err / first_err_code) so that the host can raise
 * the reference's exception for the lowest failing index, exactly as the
 * reference's sequential loop would.  Calls on one context are not re-entrant.
 */
#ifndef IKHIP_H
#define IKHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum ik_status {
  IK_OK = 0,
  IK_E_OUT_OF_REACH = 1, /* OutOfRobotReachException, kinematics/inverse.py:32 */
  IK_E_DOMAIN = 2,       /* ValueError('math domain error'), acos in inverse.py:81,92,100 */
  IK_E_ZERODIV = 3,      /* ZeroDivisionError, kinematics/point.py:40, inverse.py:81,92,100 */
  IK_E_ANGLE_RANGE = 4,  /* OutOfRobotReachException, kinematics/forward.py:23-25 */
  IK_E_BADARG = 16,      /* invalid argument (shape/size/order of calls) */
  IK_E_HIP = 17,         /* HIP runtime failure (see ik_last_error) */
  IK_E_NOMODEL = 18,     /* ik_ann_solve before ik_ann_load */
  IK_E_RCCL = 19         /* RCCL missing or a collective failed (see ik_last_error) */
} ik_status;

enum {
  IK_F_DEVICE = 1,    /* array arguments are device pointers */
  IK_F_ASYNC = 2,     /* enqueue only; requires IK_F_DEVICE */
  IK_F_NO_LIMITS = 4, /* skip the workspace check (ANN.predict has none, ann.py:70-76) */
  IK_F_PITCH_NEAREST = 8 /* ik_analytic_solve only: move an infeasible pitch to the nearest feasible */
};

enum { IK_ACT_LINEAR = 0, IK_ACT_TANH = 1, IK_ACT_RELU = 2, IK_ACT_SIGMOID = 3 };

typedef struct ik_ctx ik_ctx;

typedef struct ik_stats {
  int64_t first_oob;      /* lowest index outside the workspace limits, -1 if none */
  int64_t first_err;      /* lowest index whose solve raised, -1 if none */
  int32_t first_err_code; /* ik_status of first_err */
  int32_t max_iters;      /* FABRIK: max iterations over the batch */
  int64_t sum_iters;      /* FABRIK: total iterations */
  int64_t n_capped;       /* FABRIK: points that hit max_iter */
  double max_fk_err;      /* max |FK(theta) - p|_2 over the batch (if requested) */
  double sum_fk_err;      /* sum of |FK(theta) - p|_2 */
  double gather_ms;       /* sharded calls: the RCCL all-gather's duration (HIP events), else 0 */
} ik_stats;

/* ---- context ----------------------------------------------------------- */
/* One context per device; owns a stream, device scratch and model weights. */
int ik_ctx_create(int device, ik_ctx **out);
int ik_ctx_destroy(ik_ctx *ctx);
/* Use an external stream (e.g. torch.cuda.current_stream().cuda_stream);
 * NULL restores the context's own stream.  A context's device work is one
 * sequence whatever the streams: a call enqueued on another stream than the
 * previous call first waits (hipStreamWaitEvent) for the previous call's work,
 * so two calls never share the context's stats / work-queue words at once.
 * Host threads must still not call into one context concurrently. */
int ik_ctx_set_stream(ik_ctx *ctx, void *stream);
void *ik_ctx_get_stream(ik_ctx *ctx);
const char *ik_last_error(void); /* thread-local message of the last failure */
const char *ik_version(void);

/* ---- robot ---------------------------------------------------------------
 * robot/robot.py:38-42 SixDOFRobot: dh is the 4x4 row-major DH matrix
 * (rows thetas, d, a, alpha), links the 4 joint distances, limits
 * {x_lo, x_hi, y_lo, y_hi, z_lo, z_hi} (inclusive).  Defaults are SixDOFRobot's. */
int ik_set_robot(ik_ctx *ctx, const double *dh, const double *links, const double *limits);

/* ---- workspace check ----------------------------------------------------
 * InverseKinematics.check_limits, kinematics/inverse.py:26-35. */
int ik_check_limits(ik_ctx *ctx, const double *pts, int64_t n, int flags, ik_stats *stats);

/* ---- forward kinematics --------------------------------------------------
 * ForwardKinematics.fkine, kinematics/forward.py:73-94, batched: ang n x 4
 * (float64) -> effector xyz n x 3 and, if mats is not NULL, the four
 * cumulative transforms M_1..M_4 (n x 4 x 4 x 4, row-major; fkine's second
 * return value).  Angles outside [-2pi, 2pi] give IK_E_ANGLE_RANGE in stats. */
int ik_fk(ik_ctx *ctx, const double *ang, int64_t n, double *xyz, double *mats, int flags,
          ik_stats *stats);

/* ForwardKinematics(dh).fkine for a DH table of nj (2..1024) joints (the reference
 * takes any nj >= 3, forward.py:13-19): dh host 4 x nj row-major (thetas, d, a,
 * alpha), ang n x nj -> effector xyz n x 3 and, if mats is not NULL, the nj
 * cumulative 4 x 4 transforms (n x nj x 16; the reference's nj x nj matrices
 * are these embedded in the identity). */
int ik_fk_chain(ik_ctx *ctx, int nj, const double *dh, const double *ang, int64_t n, double *xyz,
                double *mats, int flags, ik_stats *stats);

/* ---- FABRIK ---------------------------------------------------------------
 * FabrikInverseKinematics.ikine, kinematics/inverse.py:115-139 (+ check_limits,
 * Fabrik.calculate fabrik.py:44-67, __get_angles inverse.py:54-112), batched:
 * pts n x 3 -> ang n x 4 (float64), iters n (nullable), final joint positions
 * n x 4 x 3 (nullable).  tol/max_iter: Fabrik(err_margin, max_iter_num).
 * With IK_F_DEVICE, ang must be 16-byte aligned (else IK_E_BADARG). */
int ik_fabrik_solve(ik_ctx *ctx, const double *pts, int64_t n, double tol, int32_t max_iter,
                    double *ang, int32_t *iters, double *joints, int flags, ik_stats *stats);

/* ik_fabrik_solve plus the --verbose round trip of the reference CLI
 * (cli.py:54-72, IkineCommand, the base of both --method commands): fk_err
 * (nullable) n float64 |FK(ang) - p|_2, computed in the same launch as the
 * angles; its max/sum over the finite values go to stats (max_fk_err,
 * sum_fk_err).  A point whose solve raised has fk_err NaN. */
int ik_fabrik_solve_fk(ik_ctx *ctx, const double *pts, int64_t n, double tol, int32_t max_iter,
                       double *ang, int32_t *iters, double *joints, double *fk_err, int flags,
                       ik_stats *stats);

/* Forget the context's learned FABRIK work order (the per-goal-cell cost table
 * the solves keep to start the hardest points first; DESIGN.md "Work order"):
 * the table goes back to a fresh context's -- for SixDOFRobot's chain the
 * library's built-in one (learned on random_dist batches at tol 1e-3 / 100 and
 * 1e-5 / 200; the first solve picks the one nearest its tolerance), for other
 * chains empty, i.e. point order.  Results never depend on it; only the
 * launch's tail does. */
int ik_fabrik_reset_order(ik_ctx *ctx);
/* The work-order table itself: n = 1024 cells, 1 + the largest recorded
 * iteration count per goal cell (0 = unseen).  get waits for the context's last
 * call and returns the count copied (or -ik_status); set with key NULL empties it
 * (point order). */
int ik_fabrik_order_get(ik_ctx *ctx, uint32_t *key, int n);
int ik_fabrik_order_set(ik_ctx *ctx, const uint32_t *key, int n);

/* Fabrik.calculate, kinematics/fabrik.py:44-67, batched over n goals for a chain
 * of nj (1..4096) joints: init is n x nj x 3 (or nj x 3 shared by all goals when
 * init_shared != 0), goals n x 3 -> joints n x nj x 3, iters n (nullable).
 * 2..8 joints run with the chain in registers; other lengths keep it in the
 * joints output row (same arithmetic, same bits) at about nj * max_iter * 2
 * dependent steps of ~0.4 us per goal (4096 joints x 100 iterations: ~0.3 s). */
int ik_fabrik_calc(ik_ctx *ctx, int nj, const double *dists, const double *init,
                   int init_shared, const double *goals, int64_t n, double tol,
                   int32_t max_iter, double *joints, int32_t *iters, int flags,
                   ik_stats *stats);

/* ---- ANN ----------------------------------------------------------------
 * ANN.load_model, kinematics/ann.py:78-85, with the decoded model: n_layers
 * Dense layers, dims[0..n_layers] (dims[0] == 3, dims[n_layers] == 4), acts[l]
 * one of IK_ACT_*, W[l] host float32 [dims[l]][dims[l+1]] row-major (the Keras
 * kernel layout, x @ W + b), b[l] host float32 [dims[l+1]], and the two
 * StandardScalers (ann.py:83-84).  Up to 4096 layers of widths up to 16384.
 * Up to 24 layers of widths up to 1024 run the fused kernel (one launch, the
 * activations in LDS); models wider than 512 there run its fp32 build whatever
 * ik_ann_set_mode says.  Deeper or wider models run layer at a time with the
 * activations in HBM (fp32 MFMA, one launch per layer and chunk of points,
 * still one ik_ann_solve call; ik_ann_set_mode does not apply), in chunks whose
 * two activation buffers fit IKHIP_ANN_ACT_MB (default 1024 MiB). */
int ik_ann_load(ik_ctx *ctx, int n_layers, const int32_t *dims, const int32_t *acts,
                const float *const *W, const float *const *b, const double *x_mean,
                const double *x_scale, const double *y_mean, const double *y_scale);

/* ANN.predict, kinematics/ann.py:70-76 (+ check_limits for AnnInverseKinematics.ikine,
 * inverse.py:152-155 unless IK_F_NO_LIMITS): pts n x 3 float64 -> ang n x 4
 * float32.  fk_err (nullable) n float64: |FK(ang) - p|_2, the cli.py:54-61
 * round trip, fused into the same launch; its max/sum go to stats.  With
 * IK_F_DEVICE, ang must be 16-byte aligned (else IK_E_BADARG). */
int ik_ann_solve(ik_ctx *ctx, const double *pts, int64_t n, float *ang, double *fk_err,
                 int flags, ik_stats *stats);

/* ---- Refine ------------------------------------------------------------------
 * Damped-least-squares polish of seed angles towards pts, float64, for the
 * context's robot (any DH table of 4 revolute joints).  Per row, with theta the
 * seed wrapped to [-pi, pi] (theta - 2 pi rint(theta / 2 pi)):
 *   e = p - FK(theta), err = |e|; stop when !(err > tol) or after max_iter steps;
 *   delta = J^T (J J^T + damping^2 I)^-1 e with the analytic 3 x 4 Jacobian (LDL^T);
 *   delta is scaled so that max |delta_i| <= 0.5 rad; theta = wrap(theta + delta).
 * pts n x 3, seed n x 4, ang n x 4 (float64); iters (nullable) n int32: steps
 * taken; fk_err (nullable) n float64: the error the stop test saw (<= tol for a
 * converged row, NaN for a NaN goal or seed, which takes no step).  stats:
 * max_iters / sum_iters over the rows, n_capped = rows with !(err <= tol),
 * max_fk_err / sum_fk_err over the finite errors, first_oob as for the other
 * solves (the rows are still solved); first_err stays -1.  A goal out of reach, or
 * on the line of a fully stretched seed, ends at max_iter with finite angles.
 * IK_E_BADARG: n < 0, a NULL pts / seed / ang with n > 0, max_iter < 0, tol NaN,
 * damping not finite or <= 0, IK_F_ASYNC without IK_F_DEVICE, a device ang not
 * 16-byte aligned. */
int ik_refine(ik_ctx *ctx, const double *pts, const double *seed, int64_t n, double tol,
              int32_t max_iter, double damping, double *ang, int32_t *iters /*nullable*/,
              double *fk_err /*nullable*/, int flags, ik_stats *stats);

/* ik_ann_solve, then ik_refine seeded with the network's float32 angles, in one
 * call on the context's stream: the seeds stay in device scratch.  seed_fk_err
 * (nullable): the network's own |FK - p| (what ik_ann_solve's fk_err would hold).
 * iters / fk_err nullable.  stats describe the refined result.  IK_E_NOMODEL
 * before ik_ann_load. */
int ik_ann_solve_refined(ik_ctx *ctx, const double *pts, int64_t n, double tol, int32_t max_iter,
                         double damping, double *ang, int32_t *iters, double *fk_err,
                         double *seed_fk_err, int flags, ik_stats *stats);

/* ---- Joint limits -------------------------------------------------------------
 * The robot's joint limits, per joint an interval [lo, hi] of the wrapped angle.
 * Joint i is free when lo[i] == -inf and hi[i] == +inf; otherwise it is limited and
 * needs -pi <= lo[i] <= hi[i] <= pi, both finite (lo[i] == hi[i]: a fixed joint).
 * lo == NULL and hi == NULL clear the limits; a fresh context has every joint free.
 * They are host doubles of the context, indexed by joint like the DH columns:
 * ik_set_robot does not touch them.  IK_E_BADARG, naming the joint (1..4) in
 * ik_last_error and leaving the stored limits as they were: a NaN bound, lo > hi, a
 * finite bound beyond +-pi, one infinite bound beside a finite one; also exactly one
 * NULL array.
 *
 * Only ik_refine and ik_ann_solve_refined honour them.  ik_ann_solve, the FABRIK
 * solves, ik_fk, ik_analytic_solve and the training calls ignore them: their
 * results are bit-identical whether limits are set or not (ik_check_joint_limits
 * shows what such a solve did with respect to them).
 *
 * The limited refine.  With every joint free the refine is the one above, bit for
 * bit.  With at least one limited joint, per row:
 *   theta_i = wrap(seed_i); limited i: theta_i = clip(theta_i)   (the seed, projected)
 *   repeat:
 *     e, err, J and the stop test as above (a NaN err stops at once)
 *     L = {}                                    (the joints locked for this step)
 *     solve: J' = J with the columns of L replaced by +0.0;
 *            delta = J'^T (J' J'^T + damping^2 I)^-1 e, the sums and their order as above
 *            N = {limited i not in L: (theta_i <= lo_i and delta_i < 0) or
 *                                     (theta_i >= hi_i and delta_i > 0)}
 *            N not empty: L = L + N, solve again       (at most 4 times: L only grows)
 *     delta is scaled so that max |delta_i| <= 0.5 rad
 *     free i: theta_i = wrap(theta_i + delta_i);  limited i: theta_i = clip(theta_i + delta_i)
 * with clip(t) = (t < lo_i ? lo_i : t) > hi_i ? hi_i : that (a NaN stays NaN).  Every
 * returned angle of a limited joint satisfies lo <= theta <= hi exactly.  Outputs,
 * iters, fk_err, every field of stats and NaN rows are as for the free refine.  A
 * goal that cannot be reached inside the limits ends at max_iter with finite angles
 * inside them and counts in n_capped; such a row may have every useful joint locked
 * and stand still.  A locked column adds only +0.0 terms, and clip(t) == t ==
 * wrap(t) while |t| < pi: limits that never bind give the free refine's bits. */
int ik_set_joint_limits(ik_ctx *ctx, const double *lo /*4*/, const double *hi /*4*/);
int ik_get_joint_limits(ik_ctx *ctx, double *lo /*4*/, double *hi /*4*/);
/* The rows of ang (n x 4 float64; host, or device with IK_F_DEVICE, then 16-byte
 * aligned; IK_F_ASYNC allowed with it) that break the context's joint limits: row r
 * does when for some limited joint i, with w = wrap(ang[r][i]), !(lo[i] <= w &&
 * w <= hi[i]) -- a NaN therefore does.  stats: first_err the lowest such row (-1:
 * none) with first_err_code IK_E_ANGLE_RANGE, n_capped their number, first_oob -1,
 * all else 0.  With every joint free nothing violates.  IK_E_BADARG: n < 0, a NULL
 * ang with n > 0, IK_F_ASYNC without IK_F_DEVICE. */
int ik_check_joint_limits(ik_ctx *ctx, const double *ang /*n x 4*/, int64_t n, int flags,
                          ik_stats *stats);

/* ---- Chain solve ---------------------------------------------------------------
 * Inverse kinematics of any DH table of NJ = nj (2..8) revolute joints, float64: the
 * refine above with NJ where it says 4, joint limits per joint, and restarts from
 * random points, since a general chain has no trained network to seed it.  dh (4 x nj
 * row-major: theta, d, a, alpha), lo and hi (nj each, both NULL: every joint free) are
 * always HOST pointers and are handed to the kernel by value, so an IK_F_ASYNC call
 * uploads nothing and adds no sync.  The context's robot, its workspace limits and its
 * stored joint limits are neither read nor changed: first_oob is always -1 and
 * IK_F_NO_LIMITS has no effect.  pts n x 3, seed (nullable) n x nj, ang n x nj, iters /
 * tries (nullable) n int32, fk_err (nullable) n float64 follow the usual host /
 * IK_F_DEVICE / IK_F_ASYNC convention.  Rows of ang are nj doubles; for odd nj they
 * are not 16-byte aligned, the kernel uses 8-byte accesses and this call does NOT
 * demand an aligned ang.  Per row:
 *   constants: per joint {a, d, cos alpha, sin alpha}, std::cos / std::sin on the host
 *     in float64.  Some |alpha_i| > 2 pi: every error is NaN and no row takes a step,
 *     as in ik_refine.
 *   chain: the effector Rz(t_1) B_1 .. Rz(t_NJ) B_NJ e4, B_i = Tz(d_i) Tx(a_i)
 *     Rx(alpha_i), applied right to left to a vector as a loop over the joints, the
 *     open Jacobian columns riding along: column i is (-y', x', 0) of the vector just
 *     rotated by Rz(t_i), then takes only the rotations to its left.  Column 1's z
 *     entry is identically zero and is left out of every sum.
 *   matrix: A = J' J'^T + damping^2 I, J' = J with the locked columns replaced by
 *     +0.0; each of its six entries is a sum over the joints in joint order from joint
 *     1's term (A20, A21 and A22 from joint 2's), damping^2 added last.
 *   solve: LDL^T without pivoting; delta_i = jx q0 + jy q1 + jz q2 (joint 1:
 *     jx q0 + jy q1).
 *   update: m = fmax over all |delta_i|; m > 0.5: delta = delta (0.5 / m); a free
 *     joint theta_i = wrap(theta_i + delta_i), a limited one clip(theta_i + delta_i).
 *   limits: ik_set_joint_limits' rule per joint over nj joints; the seed is projected;
 *     the active-set loop of "Joint limits" re-solves at most NJ times (on the device
 *     it is wave-uniform).
 *   seed: seed == NULL gives every row the table's theta row dh[0 .. nj-1], the home
 *     pose.
 *   restarts (0..255): attempt 0 starts from the seed.  An attempt ends like an
 *     ik_refine row: !(err > tol), or max_iter steps of this attempt.  If it ends with
 *     err > tol and attempts remain, attempt a >= 1 starts from
 *       theta_j = lo'_j + u(row, a, j) (hi'_j - lo'_j),
 *     [lo', hi'] the joint's limits or [-pi, pi] for a free joint, which then gets the
 *     seed's treatment (wrap, and clip where limited), with
 *       z = row * 0x9E3779B97F4A7C15 + ((a << 8) | j)      (uint64, wrapping; j = 0 .. nj-1)
 *       z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB
 *       z ^= z >> 31;  u = (double)(z >> 11) * 0x1p-53.
 *     A NaN error ends the row at once with no restart.  The row returns the attempt
 *     with the smallest final error, the earliest on a tie: its angles go to ang, its
 *     error to fk_err, its index to tries; iters holds the steps of all attempts
 *     together.
 * At nj = 4, restarts = 0, the result is ik_refine's for the same table and limits, bit
 * for bit.  stats: max_iters / sum_iters over iters, n_capped = rows with
 * !(fk_err <= tol), first_err the lowest such row that has a finite error with
 * first_err_code = IK_E_OUT_OF_REACH (-1: none), max_fk_err / sum_fk_err over the finite
 * errors.  Converged lanes idle until their wave's slowest row ends: restarts multiply
 * the worst row's steps, not the average's.
 * IK_E_BADARG, the context left usable: nj outside 2..8 (longer chains are not built),
 * a NULL dh, a non-finite entry in the d, a or alpha rows, the limit errors of
 * ik_set_joint_limits naming the joint, exactly one of lo / hi NULL, restarts outside
 * 0..255, max_iter (restarts + 1) above 2^31 - 1 (iters is an int32), and what ik_refine refuses (n < 0, a NULL pts / ang with n > 0, max_iter < 0,
 * tol NaN, damping not finite or <= 0, IK_F_ASYNC without IK_F_DEVICE).  n == 0 is IK_OK
 * with empty stats. */
int ik_chain_solve(ik_ctx *ctx, int nj, const double *dh /*host, 4 x nj: theta, d, a, alpha*/,
                   const double *lo /*host nj, nullable*/, const double *hi /*host nj, nullable*/,
                   const double *pts /*n x 3*/, const double *seed /*n x nj, nullable*/, int64_t n,
                   double tol, int32_t max_iter, double damping, int32_t restarts,
                   double *ang /*n x nj*/, int32_t *iters /*nullable*/, int32_t *tries /*nullable*/,
                   double *fk_err /*nullable*/, int flags, ik_stats *stats);

/* ---- Chain pose solve ----------------------------------------------------------
 * ik_chain_solve for a tool pose: position and orientation in one damped
 * least-squares step, float64, NJ = nj (2..8) revolute joints.  A goal is pts[i] (3)
 * and rot[i], a 3 x 3 matrix G, row-major, 9 doubles: the pose ik_fk_chain reports as
 * its last cumulative transform, p = M_nj[:3, 3], G = M_nj[:3, :3].  G is used as
 * given, with no orthonormalisation and no check.  dh, lo, hi, seed, ang, iters, tries,
 * the constants, the limits, the seed, the update and the start points of the restarts
 * are "Chain solve"'s; rot n x 9 and rot_err (nullable) n float64 follow the same
 * host / IK_F_DEVICE / IK_F_ASYNC convention, and no alignment is demanded.  Per row:
 *   chain: "Chain solve"'s loop, whose effector and linear columns are computed by the
 *     same operations in the same order (the same bits), with two more kinds of
 *     passenger in a second pass of the same loop.  Tool frame: three direction vectors
 *     start as the columns of Rx(alpha_NJ), (1, 0, 0), (0, ca, sa), (0, -sa, ca); they
 *     take every Rz(t_i) (vx = c x - s y, vy = s x + c y) and every Rx(alpha_i)
 *     (vy = ca y - sa z, vz = sa y + ca z) and no translation, and end as the columns
 *     r_0, r_1, r_2 of R(theta).  Axis i is opened as (0, 0, 1) when joint i is
 *     reached, where Rz(t_i) leaves it alone, and from then on takes only the rotations
 *     to its left, as linear column i does; axis 1 is identically (0, 0, 1).
 *   errors: ep = sqrt(ex^2 + ey^2 + ez^2), e = p - x, as in "Chain solve".
 *     For the step, e_w = 1/2 sum_k r_k x g_k (g_k the columns of G), sin(phi) axis in
 *     the base frame: entry m is 0.5 (((k = 0) + (k = 1)) + (k = 2)), a term being
 *     r_k[a] g_k[b] - r_k[b] g_k[a], (a, b) = (1, 2), (2, 0), (0, 1) for m = 0, 1, 2.
 *     For stopping and reporting, er = sqrt(0.5 sum_ij (R_ij - G_ij)^2), the sum
 *     row-major from (0, 0): 2 sin(phi / 2) for an orthonormal G.  The stop rule does
 *     not use |e_w|, which is zero at phi = pi.
 *   matrix: J' is 6 x NJ, rows 0..2 the linear ones, rows 3..5 w times the axes
 *     (w = rot_weight), the locked columns replaced by +0.0; e' = (e, w e_w);
 *     A = J' J'^T + damping^2 I, 21 entries, A_ij = sum_k J'_ik J'_jk over the joints in
 *     joint order from joint 1's term -- an entry of row 2, whose joint-1 value is
 *     identically zero, from joint 2's, as in "Chain solve" -- damping^2 added last on
 *     the diagonal.
 *   solve: LDL^T without pivoting,
 *       u_ij = A_ij - sum_{k<j} l_ik u_jk  (k ascending; u_jj = D_j),  l_ij = u_ij / D_j
 *       y_i = e'_i - sum_{k<i} l_ik y_k
 *       q_i = y_i / D_i - sum_{k>i} l_ki q_k  (k ascending)
 *       delta_k = sum_r J'_rk q_r  (r ascending from 0; joint 1 without r = 2)
 *     then "Chain solve"'s update and its active-set loop under limits.
 *   attempts: nan = ep or er is NaN; above = ep > tol || er > rot_tol.  An attempt ends
 *     when !above || nan || it == max_iter, and restarts when above && !nan &&
 *     a < restarts.  The row returns the attempt with the smallest score = ep + w er,
 *     the earliest on a tie (a NaN score never replaces the held one): its angles go
 *     to ang, ep to fk_err, er to rot_err, its index to tries.  Some |alpha_i| > 2 pi:
 *     both errors are NaN and no row takes a step.
 * With rot_weight = 0, rot_tol = +inf and a finite G every rotational term of the solve
 * is an exact zero, and ang, iters, tries and fk_err are ik_chain_solve's bit for bit.
 * stats: max_iters / sum_iters over iters, n_capped = rows with !(fk_err <= tol &&
 * rot_err <= rot_tol), first_err the lowest such row with both errors finite
 * (IK_E_OUT_OF_REACH; -1: none), max_fk_err / sum_fk_err over the finite position
 * errors, first_oob always -1.  Plain damped least squares on a chain that is not
 * redundant for a pose (6 joints and fewer) leaves rows stuck far from the seed;
 * restarts are the remedy and multiply the worst row's steps.
 * IK_E_BADARG, the context left usable: what ik_chain_solve refuses, a NULL rot with
 * n > 0, rot_tol NaN, rot_weight NaN, infinite or < 0.  n == 0 is IK_OK with empty
 * stats. */
int ik_chain_pose_solve(ik_ctx *ctx, int nj, const double *dh /*host, 4 x nj: theta, d, a, alpha*/,
                        const double *lo /*host nj, nullable*/, const double *hi /*host nj, nullable*/,
                        const double *pts /*n x 3*/, const double *rot /*n x 9*/,
                        const double *seed /*n x nj, nullable*/, int64_t n, double tol,
                        double rot_tol, double rot_weight, int32_t max_iter, double damping,
                        int32_t restarts, double *ang /*n x nj*/, int32_t *iters /*nullable*/,
                        int32_t *tries /*nullable*/, double *fk_err /*nullable*/,
                        double *rot_err /*nullable*/, int flags, ik_stats *stats);

/* ---- Analytic ----------------------------------------------------------------
 * Closed-form inverse kinematics with a chosen tool pitch and elbow branch, float64,
 * no iteration, for a context's robot that is a yaw joint followed by a planar
 * three-link chain: |cos alpha1| <= 1e-12 and sin alpha1 > 0, alpha2..4 = 0,
 * d2..4 = 0, a2 / a3 / a4 finite and > 0, a1 finite and >= 0 (SixDOFRobot is one;
 * any other table is IK_E_BADARG naming the entry, and the context stays usable).
 * With d1 = d[0], a1..a4 = a[0..3], per row, goal (x, y, z), elbow b = -1 / +1:
 *   theta1 = atan2(y, x);  r = sqrt(x^2 + y^2) - a1;  h = z - d1
 *   rho^2 = r^2 + h^2;  rho = sqrt(rho^2);  gamma = atan2(h, r)
 *   phi = pitch ? pitch[i] : gamma   (the tool points away from the shoulder)
 *   wrist(phi): wr = r - a4 cos phi;  wh = h - a4 sin phi;  W = sqrt(wr^2 + wh^2)
 *     m = (a2 + a3 - W)(a2 + a3 + W) / (2 a2 a3)          (= 1 - cos theta3)
 *     q = (W - |a2 - a3|)(W + |a2 - a3|) / (2 a2 a3)      (= 1 + cos theta3)
 *   infeasible = !(m >= 0 and q >= 0): the row fails, unless IK_F_PITCH_NEAREST:
 *     cmin = (rho^2 + a4^2 - (a2 + a3)^2) / (2 a4 rho)
 *     cmax = (rho^2 + a4^2 - (a2 - a3)^2) / (2 a4 rho);  delta = wrap(phi - gamma)
 *     the row fails when !(cmin <= 1 and cmax >= -1 and rho > 0), or when delta is
 *     NaN (a NaN or infinite pitch has no nearest one); else
 *     lo = acos(min(cmax, 1));  hi = acos(max(cmin, -1))
 *     phi = gamma + sign(delta) clamp(|delta|, lo, hi)   (sign(0) = +1)
 *     wrist(phi) again;  m = max(m, 0);  q = max(q, 0);  the row counts as moved
 *   s3 = b sqrt(m q);  c3 = (q - m) / 2;  theta3 = b 2 atan2(sqrt(m), sqrt(q))
 *   theta2 = atan2(wh, wr) - atan2(a3 s3, a2 + a3 c3);  theta4 = phi - theta2 - theta3
 *   ang = (theta1, wrap(theta2), theta3, wrap(theta4)), wrap as in ik_refine.
 * IK_ELBOW_UP gives theta3 <= 0, IK_ELBOW_DOWN theta3 >= 0 (the elbow below the
 * shoulder-wrist line for alpha1 = +pi/2).  Only the front branch of theta1 is
 * solved (r < 0, reaching over the back, is out of scope).
 * pts n x 3, pitch (nullable) n, ang n x 4 (float64); pitch_out (nullable) n: the
 * pitch used, bit-equal to pitch[i] on a row that was not moved; fk_err (nullable)
 * n: |FK(ang) - p|_2 through the library's FK chain, at rounding level.  A failed
 * row has ang, pitch_out and fk_err NaN.  stats: first_oob as for the other solves
 * (unless IK_F_NO_LIMITS; the rows are still solved), first_err the lowest failed
 * row with first_err_code = IK_E_OUT_OF_REACH, n_capped = rows whose pitch was
 * moved, max_iters = sum_iters = 0, max_fk_err / sum_fk_err over the finite errors.
 * IK_E_BADARG: a NULL context, n < 0, a NULL pts / ang with n > 0, elbow not -1 / +1,
 * IK_F_ASYNC without IK_F_DEVICE, a device ang not 16-byte aligned, an unsupported
 * robot.  n == 0 is IK_OK with empty stats whatever the arrays. */
enum { IK_ELBOW_UP = -1, IK_ELBOW_DOWN = 1 };
int ik_analytic_solve(ik_ctx *ctx, const double *pts, const double *pitch /*nullable: n*/,
                      int64_t n, int elbow, double *ang /*n x 4*/, double *pitch_out /*nullable*/,
                      double *fk_err /*nullable*/, int flags, ik_stats *stats);

/* Arithmetic of the hidden-layer GEMMs.  IK_ANN_FP32 (default): fp32 MFMA
 * (v_mfma_f32_32x32x2_f32), a fp32 dot product like the reference's TF/Keras
 * CPU float32 forward.  IK_ANN_BF16X6: every fp32 operand split into three bf16
 * parts and six bf16 MFMA products accumulated in fp32 -- fp32-level accuracy
 * (tested within 1e-6 of a float64 forward, the fp32 mode's own distance from
 * it) at ~2.7x the MFMA rate.  IK_ANN_FP16X3: two fp16 parts (weights
 * pre-scaled by a power of two) and three fp16 MFMA products, on layers whose
 * input is tanh/sigmoid-bounded (others stay fp32); as close to a float64
 * forward as numpy's float32 one on the tested networks, at ~5x the MFMA rate.
 * The input layer and a one-tile output layer stay fp32 in every mode.  Models
 * wider than 512 on the fused kernel stay fp32; models past its caps (the
 * layered path) run bf16x6 in either split mode.
 * Environment default: IKHIP_ANN_MODE=bf16x6|fp16x3. */
enum { IK_ANN_FP32 = 0, IK_ANN_BF16X6 = 1, IK_ANN_FP16X3 = 2 };
int ik_ann_set_mode(ik_ctx *ctx, int mode);
int ik_ann_get_mode(ik_ctx *ctx); /* the mode, or -ik_status */
/* The arithmetic the next ik_ann_solve runs for the loaded model (or
 * -ik_status; -IK_E_NOMODEL before ik_ann_load): the set mode, or IK_ANN_FP32
 * when no layer of the model can take it (a fused model wider than 512, or the
 * split planes left out at load because only the fp32 operands fit the
 * device), or IK_ANN_BF16X6 for IK_ANN_FP16X3 on the layered path. */
int ik_ann_effective_mode(ik_ctx *ctx);

/* ---- ANN training ----------------------------------------------------------
 * ANN.train_model, kinematics/ann.py:27-68: Keras' fit of a Dense stack with
 * loss 'mse' and Adam, one batch per step.  The training state (fp32 master
 * weights W[l] [dims[l]][dims[l+1]] row-major as in ik_ann_load, the Adam moments,
 * the batch's activations) is apart from the loaded inference model; a context
 * may hold both.  n_layers 1..24, every dims[l] 1..1024 (dims[0] and
 * dims[n_layers] are free here), max_batch 1..4096.  The loss of a batch is
 * sum((A_L - y)^2) / (rows dims[n_layers]), accumulated in float64; all GEMMs are
 * exact fp32 (v_mfma_f32_32x32x2_f32) with the inference kernels' activations,
 * and no reduction depends on timing: the same state and batches give the same
 * bits.  Adam is Keras': m = b1 m + (1 - b1) g, v = b2 v + (1 - b2) g^2,
 * W -= lr sqrt(1 - b2^t) / (1 - b1^t) m / (sqrt(v) + eps).  All pointers are HOST
 * pointers and every call blocks.  IK_E_BADARG: calls out of order, rows above
 * max_batch, a perm entry outside 0..n_train-1. */
int ik_ann_train_begin(ik_ctx *ctx, int n_layers, const int32_t *dims, const int32_t *acts,
                       const float *const *W, const float *const *b, int max_batch, double lr,
                       double beta1, double beta2, double eps);
/* loss = mse_weight * mse + fk_weight * fk for every later step / grads / epoch call
 * of this training state (default 1, 0: the reference's 'mse'). The four scaler
 * arrays (3, 3, 4, 4 doubles, host) are copied; they may be NULL when fk_weight == 0.
 * fk is the mean over the batch's rows of e . e, e = FK(wrap(theta)) - p in float64:
 * theta_j = a_j y_scale_j + y_mean_j from the last layer's fp32 outputs a,
 * p_k = x_k x_scale_k + x_mean_k from the row's scaled fp32 inputs, FK the chain of
 * the context's robot (NaN when some |alpha_i| > 2 pi), wrap(t) = t - 2 pi rint(t /
 * 2 pi) as in ik_refine.  Its gradient reaches the last layer as fk_weight (2 / rows)
 * (J_j . e) y_scale_j, J the analytic Jacobian, added to the mse's in float64 and
 * rounded to fp32 once.  With fk_weight > 0 one kernel replaces the loss kernel: no
 * launch is added to a step.  IK_E_BADARG (the state unchanged): before
 * ik_ann_train_begin; a negative or non-finite weight; both weights 0; with
 * fk_weight > 0, dims[0] != 3, dims[n_layers] != 4, a NULL scaler array, a non-finite
 * scaler entry or a scale of 0.  ik_ann_train_begin resets the loss to (1, 0). */
int ik_ann_train_set_loss(ik_ctx *ctx, double mse_weight, double fk_weight,
                          const double *x_mean, const double *x_scale,
                          const double *y_mean, const double *y_scale);
/* The fk term (mean squared FK error) of the last ik_ann_train_step / _grads call
 * (val_fk NaN) or of the last ik_ann_train_epoch: the steps' values weighted by their
 * rows, and the validation rows' mean (NaN without any). Both NaN while fk_weight == 0. */
int ik_ann_train_fk(ik_ctx *ctx, double *train_fk, double *val_fk);
/* The data set, already scaled: x n_train x dims[0], y n_train x dims[n_layers], and
 * the validation rows (n_val may be 0). */
int ik_ann_train_data(ik_ctx *ctx, const float *x, const float *y, int64_t n_train,
                      const float *xv, const float *yv, int64_t n_val);
/* The gradients of one batch's loss (dW[l], db[l] as W[l], b[l]); no update. */
int ik_ann_train_grads(ik_ctx *ctx, const float *x, const float *y, int rows, float *const *dW,
                       float *const *db, double *loss);
/* One Adam step on one batch; loss is the batch's loss before the update. */
int ik_ann_train_step(ik_ctx *ctx, const float *x, const float *y, int rows, double *loss);
/* One epoch over the data set in the order perm (n_train entries; NULL = data
 * order): ceil(n_train / batch) steps, the last one short.  train_loss is the
 * mean of the steps' losses weighted by their rows (Keras' running mean),
 * val_loss the loss of the end-of-epoch weights over the validation rows (NaN
 * without any). */
int ik_ann_train_epoch(ik_ctx *ctx, const int32_t *perm, int batch, double *train_loss,
                       double *val_loss);
/* Copies out what = 0 the weights and biases, 1 Adam's m, 2 Adam's v. */
int ik_ann_train_get(ik_ctx *ctx, int what, float *const *W, float *const *b);
int ik_ann_train_end(ik_ctx *ctx);

/* Per-kernel timing with HIP events: when on, every kernel a call launches
 * goes through hipExtLaunchKernel with a start and a stop event, which the
 * dispatch itself stamps (the kernel's own start and end: not the kernels ahead
 * of it on the stream, not the host's launch latency); the RCCL gather of a
 * sharded call is bracketed by stream markers.  on = 1: ik_kernel_times
 * returns the last call's kernels; on = 2: the calls' kernels accumulate, in
 * launch order, up to 64, until the next ik_ctx_set_timing (back-to-back calls
 * timed with no host sync between them).  ik_kernel_times waits for the events
 * and returns how many kernels were timed, their durations in ms and (if names
 * != NULL) their names, name_len bytes each; a negative value is -ik_status. */
int ik_ctx_set_timing(ik_ctx *ctx, int on);
int ik_kernel_times(ik_ctx *ctx, int max, float *ms, char *names, int name_len);

/* Diagnostics: when on, the ANN kernel's workgroup 0 records s_memtime stamps
 * (shader clock ticks) per wave for its first 4 tiles: 32 slots per
 * (tile, wave) -- 0 tile start, 1 input staged, 2+2l layer l GEMM done,
 * 3+2l layer l done, 31 tile done.  ik_debug_read copies them out (returns the
 * count, or -ik_status). */
int ik_ctx_set_debug(ik_ctx *ctx, int on);
int ik_debug_read(ik_ctx *ctx, uint64_t *out, int max);

/* Pinned host memory (hipHostMalloc).  A host-pointer FABRIK solve whose arrays
 * are all pinned and that has at least 131072 points (IKHIP_PIPE_MIN; 0
 * disables) is cut into chunks whose H2D copies, kernels and D2H copies overlap
 * on three streams; pageable arrays take the one-shot path. */
int ik_host_alloc(size_t bytes, void **out);
int ik_host_free(void *p);

/* After IK_F_ASYNC calls: wait for the stream and read the accumulated stats
 * of the last call. */
int ik_stats_fetch(ik_ctx *ctx, ik_stats *stats);
/* Wait for the context's last call.  With a communicator bound (ik_comm_init)
 * the wait is bounded: it polls RCCL's async error and, past the deadline
 * (ik_comm_set_timeout), aborts the communicator and returns IK_E_RCCL -- so an
 * IK_F_ASYNC caller (e.g. a benchmark loop) never hangs on a dead peer. */
int ik_ctx_sync(ik_ctx *ctx);

/* ---- multi-GPU: RCCL over xGMI ------------------------------
 * The reference scales by competing consumers of one RabbitMQ queue
 * (rpc_broker.py:55-68); here one process per GPU shares the batch instead.
 * Every rank calls the sharded solve with the same whole batch (n points, host
 * or device pointer).  The batch is cut into C chunks of g parts each
 * (ik_shard_plan): rank r solves part (c, r) = rows [(c g + r) S, (c g + r + 1) S)
 * of every chunk c (S = ceil(n / (C g)), clipped to n), writing the results at
 * their global rows of the caller's arrays, and chunk c's rows are all-gathered
 * IN PLACE (ncclAllGather with sendbuf = recvbuf + r S rows) while chunk c + 1 is
 * solved: no pack, no unpack, no padding except in the one ragged last chunk
 * (gathered through a staging buffer and copied out).  Gathered per row: the
 * angles and, for FABRIK, the iteration counts.  The per-point FK error stays
 * local: only the rank's own rows of fk_err are written; the batch's FK-error
 * max / sum / quantiles come from a 64-byte tail record (ik_shard_tail) and a
 * histogram that ride with the last chunk's all-gather, as do first_oob /
 * first_err (the lowest GLOBAL indices: the reference's sequential exception
 * precedence).  With a device pointer only the rank's own rows of pts are read.
 * RCCL is loaded at ik_comm_init (the process's librccl if already loaded --
 * torch ships one --, else librccl.so.1; IKHIP_RCCL_LIB overrides). */
#define IK_COMM_ID_BYTES 128
#define IK_MAX_GATHER_CHUNKS 8
/* FK-error histogram of a rank (uint32 counts, gathered with the tail): finite
 * e >= 0 falls in bin 16 (E - 959) + m, E the biased float64 exponent and m the top
 * 4 mantissa bits, clamped to [0, 2047] (2^-64 .. 2^64, 1/16 octave per bin). */
#define IK_FKHIST_BINS 2048

/* The stats of one rank's shard as gathered (64 bytes). */
typedef struct ik_shard_tail {
  int64_t first_oob, first_err; /* GLOBAL indices, -1 if none */
  int32_t first_err_code, max_iters;
  int64_t sum_iters, n_capped;
  double max_fk_err, sum_fk_err;
  int64_t rows; /* rows the rank solved */
} ik_shard_tail;

/* How a batch of n rows is split over nranks ranks in chunks (host only). */
typedef struct ik_shard_plan {
  int64_t n;         /* rows of the batch */
  int32_t nranks;    /* g */
  int32_t chunks;    /* C: chunks that hold rows (<= the requested count) */
  int64_t part_rows; /* S: rows of one rank's part of one chunk */
  int64_t full_rows; /* rows of the chunks gathered in place (the rest is staged) */
} ik_shard_plan;

enum { IK_METHOD_ANN = 0, IK_METHOD_FABRIK = 1 };

/* One rank creates the id and hands it to the others (any transport). */
int ik_comm_unique_id(uint8_t *id /* IK_COMM_ID_BYTES */);
/* Collective over the nranks processes: binds the context to an RCCL
 * communicator (one GPU per rank).  The communicator is non-blocking
 * (ncclCommInitRankConfig, blocking = 0): every host wait on it -- the
 * rendezvous, group ends, a synchronous call's end, ik_ctx_sync,
 * ik_stats_fetch -- polls ncclCommGetAsyncError against a deadline
 * (IKHIP_RCCL_TIMEOUT_S, default 120 s; ik_comm_set_timeout) and on an error or
 * timeout calls ncclCommAbort and returns IK_E_RCCL naming the rank and the
 * wait.  An aborted communicator (also after any failure part-way through a
 * sharded call) refuses later calls until ik_comm_destroy + ik_comm_init.  Its
 * first act is one all-gather of a 64-byte record per rank that checks the
 * ranks agree (numbering, IKHIP_GATHER_CHUNKS, library version). */
int ik_comm_init(ik_ctx *ctx, int nranks, int rank, const uint8_t *id);
/* The deadline of the communicator's waits in seconds (0: IKHIP_RCCL_TIMEOUT_S
 * or 120).  Kept across ik_comm_init. */
int ik_comm_set_timeout(ik_ctx *ctx, double seconds);
/* TEST-ONLY: a communicator without RCCL, so that one GPU can run the sharded
 * path as rank `rank` of `nranks` (the placement of every part, the ragged
 * chunk's stage, the tail reduction).  Its all-gather writes byte o of rank
 * s's slot as ik_loopback_byte(s, o) for every s != rank, and copies this
 * rank's tail block into every rank's. */
int ik_comm_init_loopback(ik_ctx *ctx, int nranks, int rank);
/* TEST-ONLY: with on != 0 the loopback communicator's all-gathers wait for a
 * peer that never comes (each block spins on a pinned flag, at most 30 s), so a
 * test can drive the deadline path: the wait times out, the abort releases the
 * flag, the GPU drains, the call returns IK_E_RCCL. */
int ik_comm_loopback_stall(ik_ctx *ctx, int on);
int ik_loopback_byte(int slot, int64_t offset);
int ik_comm_destroy(ik_ctx *ctx);
/* The communicator as the library holds it: ranks, this rank, and the chunk
 * count the last sharded call was planned with (ik_shard_plan_of's chunks; 0
 * before one), so a caller can find its own rows with ik_shard_part. */
int ik_comm_info(ik_ctx *ctx, int *nranks, int *rank, int *last_chunks);
/* Chunks per sharded call (1..IK_MAX_GATHER_CHUNKS), or 0 = automatic: one
 * chunk for both methods (one in-place all-gather after the solve; C >= 2
 * overlaps chunk c's gather with chunk c + 1's solve, opt-in until a real
 * N >= 2 run has bit-checked it).  Every rank must use the same value:
 * each call's tail carries its plan (n, chunks, method) and a rank whose plan
 * differs from rank 0's fails the call with IK_E_RCCL.  Environment default:
 * IKHIP_GATHER_CHUNKS (checked equal on every rank by ik_comm_init). */
int ik_comm_set_chunks(ik_ctx *ctx, int chunks);
/* Host-only helpers of the protocol (no device needed). */
int ik_shard_plan_of(int64_t n, int nranks, int chunks, ik_shard_plan *out);
/* Rank's part of chunk c: rows [begin, end) (empty when begin == end). */
int ik_shard_part(const ik_shard_plan *plan, int rank, int chunk, int64_t *begin, int64_t *end);
/* = ik_shard_part of the one-chunk plan: rank's rows [r S, (r + 1) S) clipped, S = ceil(n / g). */
int ik_shard_range(int64_t n, int nranks, int rank, int64_t *begin, int64_t *end);
int ik_tail_reduce(const ik_shard_tail *tails, int nranks, ik_stats *out);
/* The bin of an FK error (see IK_FKHIST_BINS; -1 for NaN / inf / negative) and
 * the upper edge of a bin. */
int ik_fkhist_bin(double e);
double ik_fkhist_upper(int bin);
/* q-quantile (0 < q <= 1) of the FK errors of the last sharded call, from the
 * gathered histograms: the upper edge of the bin holding the ceil(q m)-th
 * smallest of the m finite errors (an upper bound, within 1/16 octave).  Needs
 * fk_err in that call; waits for it. */
int ik_fk_err_quantile(ik_ctx *ctx, double q, double *out);

/* AnnInverseKinematics.ikine / ANN.predict (see ik_ann_solve) over the ranks:
 * ang n x 4 float32 of the WHOLE batch; fk_err (nullable) n float64, of which
 * only this rank's rows are written. */
int ik_ann_solve_sharded(ik_ctx *ctx, const double *pts, int64_t n, float *ang, double *fk_err,
                         int flags, ik_stats *stats);
/* FabrikInverseKinematics.ikine (see ik_fabrik_solve_fk) over the ranks: ang n x 4
 * float64 and iters (nullable) n int32 of the whole batch, fk_err (nullable) n
 * float64 of this rank's rows. */
int ik_fabrik_solve_sharded(ik_ctx *ctx, const double *pts, int64_t n, double tol,
                            int32_t max_iter, double *ang, int32_t *iters, double *fk_err,
                            int flags, ik_stats *stats);

#ifdef __cplusplus
}
#endif
#endif /* IKHIP_H */
