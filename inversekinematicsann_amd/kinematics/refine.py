"""Damped-least-squares refine of IK seed angles -- the numpy restatement of
libikhip's ik_refine (csrc/ik_refine.hip), importable without the native library.

For one goal p and seed theta_0 (4 revolute joints of a DH table):

    theta <- wrap(theta_0)                  # theta - 2 pi rint(theta / 2 pi)
    repeat:
        e   <- p - FK(theta);  err <- sqrt(e . e)
        stop if !(err > tol) or it == max_iter       # a NaN err stops at once
        J   <- dFK / dtheta  (3 x 4, analytic)
        A   <- J J^T + damping^2 I                   # SPD; LDL^T, no pivoting
        d   <- J^T A^-1 e
        m   <- max |d_i|;  if m > STEP_CLAMP: d <- d (STEP_CLAMP / m)
        theta <- wrap(theta + d);  it <- it + 1

refine_reference follows the kernel operation for operation -- the same chain
(csrc/ik_chain_jac.h, restated by _chain_cs: the effector as
Rz(t1) B1 Rz(t2) B2 Rz(t3) B3 Rz(t4) B4 e4 applied right to left,
B_i = Tz(d_i) Tx(a_i) Rx(alpha_i)), the same sums in the same order, no fused
multiply-add -- so in float64 it differs from the kernel only by the kernel's
sin / cos (within 1.2e-16 of libm's).

With joint limits (ik_set_joint_limits; refine_reference(joint_limits=...)) a limited
joint's angle is pulled into [lo, hi] where a free one is wrapped -- the seed too --
and d comes from an active-set loop: a limited joint on a bound whose d_i points
out of the interval has its column of J replaced by +0.0 and the system is solved
again, until no new joint locks (csrc/ik_refine_step.h, restated by _solve and
_limited_step).  joint_limit_violations is the twin of ik_check_joint_limits.

Known limits: a goal outside reach, or on the line of a fully stretched seed
(fixed damping does not leave that singular direction), ends at max_iter with
finite angles and err > tol.
"""
from __future__ import annotations

import numpy as np

STEP_CLAMP = 0.5  # largest |delta_i| of one step, radians
DEFAULT_TOL, DEFAULT_MAX_ITER, DEFAULT_DAMPING = 1e-6, 20, 1e-3


def _consts(dh, dtype):
    """Per joint a_i, d_i, cos alpha_i, sin alpha_i (the library's fk_trip_consts,
    computed in float64 as there) and whether some |alpha_i| > 2 pi."""
    dh = np.asarray(dh, np.float64).reshape(4, 4)
    al = dh[3]
    a, d = dh[2].astype(dtype), dh[1].astype(dtype)
    ca, sa = np.cos(al).astype(dtype), np.sin(al).astype(dtype)
    return a, d, ca, sa, bool(np.any((al < -2 * np.pi) | (al > 2 * np.pi)))


def wrap(theta, dtype=np.float64):
    """theta - 2 pi rint(theta / 2 pi), in [-pi, pi]."""
    t = np.asarray(theta, dtype)
    two_pi = dtype(2 * np.pi)
    return t - two_pi * np.rint(t / two_pi)


def _chain(consts, th):
    """The effector (x, y, z) and the Jacobian's columns [(jx, jy, jz)] * 4 of the
    angle rows th (n x 4): _chain_cs on numpy's sines and cosines."""
    return _chain_cs(consts, np.sin(th), np.cos(th))


def _chain_cs(consts, s, c):
    """The same from the angles' sines and cosines (n x 4 each): the sequence of
    csrc/ik_chain_jac.h fk_chain_jac, which the refine kernel and the training loss's
    FK term both call."""
    a, d, ca, sa, _ = consts
    n, dtype = s.shape[0], s.dtype
    x = np.full(n, a[3], dtype)
    y = np.zeros(n, dtype)
    z = np.full(n, d[3], dtype)
    cols = []  # open columns, the latest joint first
    for i in (3, 2, 1, 0):
        ci, si = c[:, i], s[:, i]
        xr = ci * x - si * y
        yr = si * x + ci * y
        for w in cols:  # Rz(t_i) on the columns to its right
            wx = ci * w[0] - si * w[1]
            wy = si * w[0] + ci * w[1]
            w[0], w[1] = wx, wy
        cols.append([-yr, xr, np.zeros(n, dtype)])  # d Rz(t_i) v / dt_i
        x, y = xr, yr
        if i > 0:  # B_i (1-based): Rx(alpha), then the translations (a, 0, d)
            b = i - 1
            yb = ca[b] * y - sa[b] * z
            zb = sa[b] * y + ca[b] * z + d[b]
            x = x + a[b]
            y, z = yb, zb
            for w in cols:
                wy = ca[b] * w[1] - sa[b] * w[2]
                wz = sa[b] * w[1] + ca[b] * w[2]
                w[1], w[2] = wy, wz
    j3, j2, j1, j0 = cols
    return (x, y, z), (j0, j1, j2, j3)


def jacobian(dh, ang):
    """dFK / dtheta of the DH chain at ang (n x 4 or 4): n x 3 x 4 float64."""
    th = np.asarray(ang, np.float64).reshape(-1, 4)
    _, J = _chain(_consts(dh, np.float64), th)
    return np.stack([np.stack(col, axis=1) for col in J], axis=2)


def joint_limit_arrays(joint_limits):
    """(lo, hi), two float64 arrays of 4 with -inf / +inf for a free joint, from None
    (every joint free), a pair (lo[4], hi[4]) or four entries, each (lo, hi) or None.
    The library's refusals (ik_set_joint_limits) as ValueError naming the joint."""
    lo, hi = np.full(4, -np.inf), np.full(4, np.inf)
    if joint_limits is None:
        return lo, hi
    jl = list(joint_limits)
    if len(jl) == 2 and all(e is not None and np.shape(e) == (4,) for e in jl):
        lo, hi = np.array(jl[0], np.float64), np.array(jl[1], np.float64)
    elif len(jl) == 4:
        for i, e in enumerate(jl):
            if e is not None:
                lo[i], hi[i] = (float(v) for v in e)
    else:
        raise ValueError("joint_limits: four entries, each (lo, hi) or None, or a pair "
                         "(lo[4], hi[4])")
    for i in range(4):
        who = f"joint_limits: joint {i + 1}: "
        if np.isnan(lo[i]) or np.isnan(hi[i]):
            raise ValueError(who + "a bound is NaN")
        if lo[i] == -np.inf and hi[i] == np.inf:
            continue
        if np.isinf(lo[i]) != np.isinf(hi[i]):
            raise ValueError(who + "one bound is infinite and the other finite")
        if lo[i] > hi[i]:
            raise ValueError(who + "lo > hi")
        if lo[i] < -np.pi or hi[i] > np.pi:
            raise ValueError(who + "a bound lies outside [-pi, pi]")
    return lo, hi


def joint_limit_violations(ang, joint_limits):
    """The numpy twin of ik_check_joint_limits: one bool per row of ang (n x 4), true
    when some limited joint's wrapped angle w has !(lo <= w <= hi) (a NaN has)."""
    lo, hi = joint_limit_arrays(joint_limits)
    limited = ~((lo == -np.inf) & (hi == np.inf))
    w = wrap(np.asarray(ang, np.float64).reshape(-1, 4))
    with np.errstate(invalid="ignore"):
        return (~((lo <= w) & (w <= hi)) & limited).any(axis=1)


def _project(t, lo, hi):
    """ik_refine_step.h refine_project: t pulled into [lo, hi], a NaN stays NaN."""
    t = np.where(t < lo, lo, t)
    return np.where(t > hi, hi, t)


def _solve(J, e, lam2, lock):
    """ik_refine_step.h refine_solve: delta (4 arrays) = J'^T (J' J'^T + lam2 I)^-1 e
    with the columns lock[:, i] of J replaced by +0.0 (lock None: none)."""
    j0, j1, j2, j3 = J
    if lock is not None:
        zero = np.zeros_like(e[0])
        j0, j1, j2, j3 = ([np.where(lock[:, i], zero, c) for c in col]
                          for i, col in enumerate(J))
    ex, ey, ez = e
    A00 = j0[0] * j0[0] + j1[0] * j1[0] + j2[0] * j2[0] + j3[0] * j3[0] + lam2
    A10 = j0[1] * j0[0] + j1[1] * j1[0] + j2[1] * j2[0] + j3[1] * j3[0]
    A11 = j0[1] * j0[1] + j1[1] * j1[1] + j2[1] * j2[1] + j3[1] * j3[1] + lam2
    A20 = j1[2] * j1[0] + j2[2] * j2[0] + j3[2] * j3[0]
    A21 = j1[2] * j1[1] + j2[2] * j2[1] + j3[2] * j3[1]
    A22 = j1[2] * j1[2] + j2[2] * j2[2] + j3[2] * j3[2] + lam2
    l10, l20 = A10 / A00, A20 / A00
    D1 = A11 - l10 * A10
    u21 = A21 - l20 * A10
    l21 = u21 / D1
    D2 = A22 - l20 * A20 - l21 * u21
    y1 = ey - l10 * ex
    y2 = ez - l20 * ex - l21 * y1
    q2 = y2 / D2
    q1 = y1 / D1 - l21 * q2
    q0 = ex / A00 - l10 * q1 - l20 * q2
    e0 = j0[0] * q0 + j0[1] * q1
    e1 = j1[0] * q0 + j1[1] * q1 + j1[2] * q2
    e2 = j2[0] * q0 + j2[1] * q1 + j2[2] * q2
    e3 = j3[0] * q0 + j3[1] * q1 + j3[2] * q2
    return e0, e1, e2, e3


def _limited_step(J, e, lam2, th, lo, hi, limited):
    """ik_refine_step.h refine_step on every row: (delta, lock n x 4 bool, re-solves
    per row).  As in the kernel's wave, all rows solve again while any row has a new
    lock; a row with nothing new gets the same values."""
    n = th.shape[0]
    lock = np.zeros((n, 4), bool)
    resolves = np.zeros(n, np.int32)
    while True:
        d = _solve(J, e, lam2, lock)
        dd = np.stack(d, axis=1)
        new = (((th <= lo) & (dd < 0)) | ((th >= hi) & (dd > 0))) & limited & ~lock
        lock = lock | new
        grew = new.any(axis=1)
        resolves = resolves + grew.astype(np.int32)
        if not grew.any():
            return d, lock, resolves


def refine_reference(pts, seed, tol=DEFAULT_TOL, max_iter=DEFAULT_MAX_ITER,
                     damping=DEFAULT_DAMPING, dh=None, dtype=np.float64, joint_limits=None,
                     trace=None):
    """The refine of every (pts[i], seed[i]); returns (theta n x 4, iters n int32,
    err n) in dtype (np.float64 or np.longdouble).

    joint_limits: None, or what joint_limit_arrays takes ((lo, hi) with -inf / +inf
    for a free joint).  With at least one limited joint the step is the library's
    limited refine (include/ikhip.h "Joint limits"), restated operation for operation;
    with none the code path is the free one.

    trace: a list that receives one dict per step of the limited refine -- the rows
    that took it (rows), J (11 columns: j0x j0y j1x .. j3z), e, theta before the step,
    delta before the 0.5 rad scaling, the lock mask (bits) and the re-solves."""
    if dh is None:
        from ..robot.robot import SixDOFRobot
        dh = SixDOFRobot.dh_matrix
    dtype = np.dtype(dtype).type
    consts = _consts(dh, dtype)
    p = np.asarray(pts, dtype).reshape(-1, 3)
    th = wrap(np.asarray(seed, dtype).reshape(-1, 4), dtype)
    lo64, hi64 = joint_limit_arrays(joint_limits)
    limited = ~((lo64 == -np.inf) & (hi64 == np.inf))
    lo, hi = lo64.astype(dtype), hi64.astype(dtype)
    if limited.any():
        th = np.where(limited, _project(th, lo, hi), th)
    n = p.shape[0]
    tol = dtype(tol)
    lam2 = dtype(np.float64(damping) * np.float64(damping))
    clamp = dtype(STEP_CLAMP)
    it = np.zeros(n, np.int32)
    err = np.zeros(n, dtype)
    active = np.ones(n, bool)
    with np.errstate(all="ignore"):
        while n:
            (x, y, z), J = _chain(consts, th)
            ex, ey, ez = p[:, 0] - x, p[:, 1] - y, p[:, 2] - z
            en = np.sqrt(ex * ex + ey * ey + ez * ez)
            if consts[4]:
                en = np.full(n, np.nan, dtype)
            err = np.where(active, en, err)
            active = active & ~(~(err > tol) | (it == max_iter))
            if not active.any():
                break
            if limited.any():
                (e0, e1, e2, e3), lock, resolves = _limited_step(J, (ex, ey, ez), lam2, th, lo,
                                                                 hi, limited)
                if trace is not None:
                    rows = np.flatnonzero(active)
                    cols = [J[0][0], J[0][1]] + [c for col in J[1:] for c in col]
                    trace.append({
                        "rows": rows, "J": np.stack(cols, axis=1)[rows],
                        "e": np.stack([ex, ey, ez], axis=1)[rows], "theta": th[rows],
                        "delta": np.stack([e0, e1, e2, e3], axis=1)[rows],
                        "lock": (lock[rows] << np.arange(4)).sum(axis=1),
                        "resolves": resolves[rows]})
            else:
                e0, e1, e2, e3 = _solve(J, (ex, ey, ez), lam2, None)
            m = np.fmax(np.fmax(np.abs(e0), np.abs(e1)), np.fmax(np.abs(e2), np.abs(e3)))
            big = m > clamp
            sc = np.where(big, clamp / np.where(big, m, 1), 1)
            d = np.stack([np.where(big, e * sc, e) for e in (e0, e1, e2, e3)], axis=1)
            if limited.any():
                new = np.where(limited, _project(th + d, lo, hi), wrap(th + d, dtype))
            else:
                new = wrap(th + d, dtype)
            th = np.where(active[:, None], new, th)
            it = it + active.astype(np.int32)
    return th, it, err
