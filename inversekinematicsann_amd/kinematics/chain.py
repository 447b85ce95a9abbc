"""Inverse kinematics of any DH chain of 2..8 revolute joints: damped least squares
with joint limits and random restarts -- the numpy restatement of libikhip's
ik_chain_solve (csrc/ik_chain.hip, csrc/ik_chain_row.h) and the class that calls
it.  Importable without the native library.

It is kinematics/refine.py with nj where that says 4, plus restarts.  Per row:

    attempt 0 starts from place(seed)          # wrap; a limited joint is clipped
    an attempt is refine.py's loop: stop when !(err > tol) or after max_iter steps
    it ends with err > tol and attempts remain: attempt a starts from
        place(lo'_j + u(row, a, j) (hi'_j - lo'_j))   # [lo', hi']: the joint's limits,
                                                     # or [-pi, pi] for a free joint
    a NaN err ends the row with no restart
    the row returns the attempt with the smallest final err, the earliest on a tie

chain_refine_reference follows the kernel operation for operation (the chain and
the sums over the joints in joint order, no fused multiply-add, the start-point
hash in uint64), so in float64 it differs from the kernel only by the kernel's
sin / cos (within 1.2e-16 of libm's).  At nj = 4 and restarts = 0 it gives
refine_reference's bits.

chain_pose_reference restates ik_chain_pose_solve (csrc/ik_chain_pose_row.h) the same
way: the goal is a position and a 3 x 3 rotation, the step one 6-row damped least squares
on the linear and the angular Jacobian, an attempt stops on the position error and on
the chord sqrt(1/2 |R - G|_F^2) = 2 sin(phi / 2).  With rot_weight = 0 and rot_tol = inf
it gives chain_refine_reference's bits.  Plain damped least squares on a chain that is
not redundant for a pose (6 joints and fewer) is a local method: far from the seed many
rows end above tol, and restarts help less than for a point.

Known cost: a general chain has no trained network to seed it, and plain damped
least squares from the home pose leaves rows stuck (a 3-joint chain is not
redundant: hundreds of rows of a few thousand; 6 and 7 joints: a few).  Restarts
from uniform points are the remedy; they multiply the worst row's steps.
"""
from __future__ import annotations

import numpy as np

from .refine import STEP_CLAMP, _project, wrap

MIN_JOINTS, MAX_JOINTS = 2, 8
MAX_RESTARTS = 255
DEFAULT_TOL, DEFAULT_MAX_ITER, DEFAULT_DAMPING, DEFAULT_RESTARTS = 1e-6, 60, 1e-3, 4


def chain_dh(dh):
    """The DH table as float64 4 x nj (rows theta, d, a, alpha) with the library's
    refusals (ik_chain_solve) as ValueError."""
    d = np.array(dh, np.float64)
    if d.ndim != 2 or d.shape[0] != 4:
        raise ValueError("dh must be 4 x nj (rows theta, d, a, alpha)")
    nj = d.shape[1]
    if not MIN_JOINTS <= nj <= MAX_JOINTS:
        raise ValueError(f"dh has {nj} joints: ik_chain_solve takes {MIN_JOINTS}..{MAX_JOINTS} "
                         "(longer chains are not built)")
    if not np.isfinite(d[1:]).all():
        raise ValueError("dh: a non-finite entry in the d, a or alpha rows")
    return d


def check_steps(max_iter, restarts):
    """The library's refusals of max_iter and restarts: restarts 0..255, max_iter >= 0,
    and max_iter (restarts + 1), the most steps a row's int32 count can hold, at most
    2^31 - 1."""
    if not 0 <= int(restarts) <= MAX_RESTARTS:
        raise ValueError(f"restarts must be 0..{MAX_RESTARTS}")
    if int(max_iter) < 0:
        raise ValueError("max_iter must be >= 0")
    if int(max_iter) * (int(restarts) + 1) > 2 ** 31 - 1:
        raise ValueError("max_iter * (restarts + 1) must not exceed 2^31 - 1, the steps a row "
                         "can count")


def _consts(dh, dtype):
    """Per joint a_i, d_i, cos alpha_i, sin alpha_i (computed in float64 as the
    library's host code does) and whether some |alpha_i| > 2 pi."""
    dh = np.asarray(dh, np.float64)
    al = dh[3]
    a, d = dh[2].astype(dtype), dh[1].astype(dtype)
    ca, sa = np.cos(al).astype(dtype), np.sin(al).astype(dtype)
    return a, d, ca, sa, bool(np.any((al < -2 * np.pi) | (al > 2 * np.pi)))


def _chain(consts, th):
    return _chain_cs(consts, np.sin(th), np.cos(th))


def _chain_cs(consts, s, c):
    """The effector (x, y, z) and the Jacobian's columns [[jx, jy, jz]] * nj from the
    angles' sines and cosines (n x nj each): csrc/ik_chain_row.h chain_jac."""
    a, d, ca, sa, _ = consts
    n, nj, dtype = s.shape[0], s.shape[1], s.dtype
    x = np.full(n, a[nj - 1], dtype)
    y = np.zeros(n, dtype)
    z = np.full(n, d[nj - 1], dtype)
    cols = []  # open columns, the latest joint first
    for i in range(nj - 1, -1, -1):
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
    return (x, y, z), cols[::-1]


def chain_fk(dh, ang):
    """The effector of the DH chain at ang (n x nj or nj): n x 3 float64, through the
    restatement's chain."""
    dh = np.asarray(dh, np.float64)
    th = np.asarray(ang, np.float64).reshape(-1, dh.shape[1])
    (x, y, z), _ = _chain(_consts(dh, np.float64), th)
    return np.stack([x, y, z], axis=1)


def chain_jacobian(dh, ang):
    """dFK / dtheta of the DH chain at ang (n x nj or nj): n x 3 x nj float64."""
    dh = np.asarray(dh, np.float64)
    th = np.asarray(ang, np.float64).reshape(-1, dh.shape[1])
    _, J = _chain(_consts(dh, np.float64), th)
    return np.stack([np.stack(col, axis=1) for col in J], axis=2)


def chain_limit_arrays(joint_limits, nj):
    """(lo, hi), two float64 arrays of nj with -inf / +inf for a free joint, from
    None (every joint free), a pair of numpy arrays (lo[nj], hi[nj]), or nj entries,
    each a tuple or list (lo, hi) or None.  The two forms are told apart by type, not
    by length, so that a 2-joint chain is no special case: two numpy arrays are the
    pair, anything else is per joint.  The library's refusals (ik_set_joint_limits'
    rule per joint) as ValueError naming the joint."""
    lo, hi = np.full(nj, -np.inf), np.full(nj, np.inf)
    if joint_limits is None:
        return lo, hi
    jl = list(joint_limits)
    shape = f"{nj} entries, each (lo, hi) or None, or a pair of arrays (lo[{nj}], hi[{nj}])"
    if len(jl) == 2 and any(isinstance(e, np.ndarray) for e in jl):
        if not all(isinstance(e, np.ndarray) for e in jl):
            raise ValueError("joint_limits: lo and hi must both be given (two numpy arrays)")
        if any(e.shape != (nj,) for e in jl):
            raise ValueError("joint_limits: " + shape)
        lo, hi = np.array(jl[0], np.float64), np.array(jl[1], np.float64)
    elif len(jl) == nj:
        for i, e in enumerate(jl):
            if isinstance(e, np.ndarray):
                raise ValueError("joint_limits: joint %d: an entry is a tuple or list (lo, hi) "
                                 "or None; numpy arrays are the pair (lo[nj], hi[nj])" % (i + 1))
            if e is not None:
                lo[i], hi[i] = (float(v) for v in e)
    else:
        raise ValueError("joint_limits: " + shape)
    for i in range(nj):
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


def start_u(rows, a, j):
    """csrc/ik_chain_row.h chain_start_u: the uniform float64 in [0, 1) of (row,
    attempt a, joint j), rows an integer array."""
    with np.errstate(over="ignore"):
        z = np.asarray(rows).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15) \
            + np.uint64((int(a) << 8) | int(j))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def _solve(J, e, lam2, lock):
    """chain_solve: delta (nj arrays) = J'^T (J' J'^T + lam2 I)^-1 e with the columns
    lock[:, i] of J replaced by +0.0 (lock None: none)."""
    if lock is not None:
        zero = np.zeros_like(e[0])
        J = [[np.where(lock[:, i], zero, c) for c in col] for i, col in enumerate(J)]
    nj = len(J)
    ex, ey, ez = e
    A00, A10, A11 = J[0][0] * J[0][0], J[0][1] * J[0][0], J[0][1] * J[0][1]
    A20, A21, A22 = J[1][2] * J[1][0], J[1][2] * J[1][1], J[1][2] * J[1][2]
    for k in range(1, nj):
        A00 = A00 + J[k][0] * J[k][0]
        A10 = A10 + J[k][1] * J[k][0]
        A11 = A11 + J[k][1] * J[k][1]
    for k in range(2, nj):
        A20 = A20 + J[k][2] * J[k][0]
        A21 = A21 + J[k][2] * J[k][1]
        A22 = A22 + J[k][2] * J[k][2]
    A00, A11, A22 = A00 + lam2, A11 + lam2, A22 + lam2
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
    out = [J[0][0] * q0 + J[0][1] * q1]
    for k in range(1, nj):
        out.append(J[k][0] * q0 + J[k][1] * q1 + J[k][2] * q2)
    return out


def _limited_step(J, e, lam2, th, lo, hi, limited):
    """chain_step on every row: (delta, lock n x nj bool, re-solves per row).  All rows
    solve again while any row has a new lock; a row with nothing new gets the same
    values."""
    n, nj = th.shape
    lock = np.zeros((n, nj), bool)
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


def _place(th, lo, hi, limited, dtype):
    """chain_place: a limited joint is clipped, a free one wrapped."""
    w = wrap(th, dtype)
    if limited.any():
        return np.where(limited, _project(w, lo, hi), w)
    return w


def _update(th, d, lo, hi, limited, dtype):
    """chain_scale, then chain_place of theta + delta: delta scaled so that max
    |delta_i| <= 0.5 rad; a free joint wrapped, a limited one clipped."""
    clamp = dtype(STEP_CLAMP)
    m = np.abs(d[0])
    for e in d[1:]:
        m = np.fmax(m, np.abs(e))
    big = m > clamp
    sc = np.where(big, clamp / np.where(big, m, 1), 1)
    dd = np.stack([np.where(big, e * sc, e) for e in d], axis=1)
    if limited.any():
        return np.where(limited, _project(th + dd, lo, hi), wrap(th + dd, dtype))
    return wrap(th + dd, dtype)


def _attempt(consts, p, th, tol, max_iter, lam2, lo, hi, limited, dtype, trace=None):
    """One attempt of every row from the placed angles th: (theta, steps, err)."""
    n = p.shape[0]
    it = np.zeros(n, np.int32)
    err = np.zeros(n, dtype)
    active = np.ones(n, bool)
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
            d, lock, resolves = _limited_step(J, (ex, ey, ez), lam2, th, lo, hi, limited)
            if trace is not None:
                rows = np.flatnonzero(active)
                trace.append({
                    "rows": rows, "theta": th[rows],
                    "e": np.stack([ex, ey, ez], axis=1)[rows],
                    "delta": np.stack(d, axis=1)[rows],
                    "lock": (lock[rows].astype(np.int64) << np.arange(th.shape[1])).sum(axis=1),
                    "resolves": resolves[rows]})
        else:
            d = _solve(J, (ex, ey, ez), lam2, None)
        th = np.where(active[:, None], _update(th, d, lo, hi, limited, dtype), th)
        it = it + active.astype(np.int32)
    return th, it, err


def chain_refine_reference(pts, seed, tol=DEFAULT_TOL, max_iter=DEFAULT_MAX_ITER,
                           damping=DEFAULT_DAMPING, dh=None, joint_limits=None, restarts=0,
                           dtype=np.float64, trace=None):
    """ik_chain_solve of every (pts[i], seed[i]) on the DH table dh (4 x nj); seed
    None: the table's theta row for every row.  Returns (theta n x nj, iters n int32:
    the steps of all attempts, tries n int32: the returned attempt, err n) in dtype
    (np.float64 or np.longdouble).  trace: a list that receives one dict per step of
    attempt 0 under limits (rows, theta, e, delta before the scaling, lock, resolves)."""
    dh = chain_dh(dh)
    nj = dh.shape[1]
    check_steps(max_iter, restarts)
    dtype = np.dtype(dtype).type
    consts = _consts(dh, dtype)
    p = np.asarray(pts, dtype).reshape(-1, 3)
    n = p.shape[0]
    lo64, hi64 = chain_limit_arrays(joint_limits, nj)
    limited = ~((lo64 == -np.inf) & (hi64 == np.inf))
    lo, hi = lo64.astype(dtype), hi64.astype(dtype)
    if seed is None:
        seed = np.tile(dh[0], (n, 1))
    tol = dtype(tol)
    lam2 = dtype(np.float64(damping) * np.float64(damping))
    # [lo', hi'] of the start points
    pi = dtype(np.float64(3.141592653589793))
    slo, shi = np.where(limited, lo, -pi), np.where(limited, hi, pi)
    with np.errstate(all="ignore"):
        th0 = _place(np.asarray(seed, dtype).reshape(-1, nj), lo, hi, limited, dtype)
        best_th, tot, best_err = _attempt(consts, p, th0, tol, max_iter, lam2, lo, hi, limited,
                                          dtype, trace)
        tries = np.zeros(n, np.int32)
        last_err = best_err
        rows = np.arange(n)
        for a in range(1, int(restarts) + 1):
            keep = last_err > tol  # (a NaN error does not restart)
            rows, last_err = rows[keep], last_err[keep]
            if rows.size == 0:
                break
            u = np.stack([start_u(rows, a, j) for j in range(nj)], axis=1).astype(dtype)
            start = _place(slo + u * (shi - slo), lo, hi, limited, dtype)
            th, it, last_err = _attempt(consts, p[rows], start, tol, max_iter, lam2, lo, hi,
                                        limited, dtype)
            tot[rows] += it
            better = last_err < best_err[rows]
            w = rows[better]
            best_th[w], best_err[w], tries[w] = th[better], last_err[better], a
    return best_th, tot, tries, best_err


# ---- pose goals: csrc/ik_chain_pose_row.h, ik_chain_pose_solve ------------------------
def _pose_frame_cs(consts, s, c):
    """pose_jac's second pass: the tool frame's columns [[x, y, z]] * 3 and the joint
    axes [[wx, wy, wz]] * nj from the angles' sines and cosines."""
    a, d, ca, sa, _ = consts
    n, nj, dtype = s.shape[0], s.shape[1], s.dtype
    zero, one = np.zeros(n, dtype), np.ones(n, dtype)
    can, san = np.full(n, ca[nj - 1], dtype), np.full(n, sa[nj - 1], dtype)
    r = [[one, zero, zero], [zero, can, san], [zero, -san, can]]
    axes = []  # open axes, the latest joint first
    for i in range(nj - 1, -1, -1):
        ci, si = c[:, i], s[:, i]
        for v in r + axes:  # Rz(t_i) on the frame and on the axes to its right
            vx = ci * v[0] - si * v[1]
            vy = si * v[0] + ci * v[1]
            v[0], v[1] = vx, vy
        axes.append([zero, zero, one])
        if i > 0:  # Rx(alpha_i) (1-based); the translations move no direction
            b = i - 1
            for v in r + axes:
                vy = ca[b] * v[1] - sa[b] * v[2]
                vz = sa[b] * v[1] + ca[b] * v[2]
                v[1], v[2] = vy, vz
    return r, axes[::-1]


def _rot_step_error(r, G):
    """pose_rot_step_error: e_w = 1/2 sum_k r_k x g_k, three arrays; G n x 9 row-major."""
    out = []
    for m in range(3):
        a, b = (m + 1) % 3, (m + 2) % 3
        acc = r[0][a] * G[:, 3 * b] - r[0][b] * G[:, 3 * a]
        for k in (1, 2):
            acc = acc + (r[k][a] * G[:, 3 * b + k] - r[k][b] * G[:, 3 * a + k])
        out.append(acc.dtype.type(0.5) * acc)
    return out


def _rot_error(r, G):
    """pose_rot_error: sqrt(1/2 sum_ij (R_ij - G_ij)^2), the sum row-major."""
    acc = None
    for i in range(3):
        for j in range(3):
            v = r[j][i] - G[:, 3 * i + j]
            acc = v * v if acc is None else acc + v * v
    return np.sqrt(acc.dtype.type(0.5) * acc)


def _pose_solve(J, W, e, w, lam2, lock):
    """pose_solve: delta (nj arrays) from the linear columns J, the axes W, e' (six
    arrays, the last three already times w), the columns lock[:, i] replaced by +0.0."""
    nj = len(J)
    rows = [[J[k][0] for k in range(nj)], [J[k][1] for k in range(nj)],
            [J[k][2] for k in range(nj)], [w * W[k][0] for k in range(nj)],
            [w * W[k][1] for k in range(nj)], [w * W[k][2] for k in range(nj)]]
    if lock is not None:
        zero = np.zeros_like(e[0])
        rows = [[np.where(lock[:, k], zero, row[k]) for k in range(nj)] for row in rows]
    u = [[None] * 6 for _ in range(6)]
    for i in range(6):
        for j in range(i + 1):
            k0 = 1 if (i == 2 or j == 2) else 0
            acc = rows[i][k0] * rows[j][k0]
            for k in range(k0 + 1, nj):
                acc = acc + rows[i][k] * rows[j][k]
            u[i][j] = acc + lam2 if i == j else acc
    low = [[None] * 6 for _ in range(6)]
    D = [None] * 6
    for j in range(6):
        for i in range(j, 6):
            for k in range(j):
                u[i][j] = u[i][j] - low[i][k] * u[j][k]
        D[j] = u[j][j]
        for i in range(j + 1, 6):
            low[i][j] = u[i][j] / D[j]
    y, q = [None] * 6, [None] * 6
    for i in range(6):
        y[i] = e[i]
        for k in range(i):
            y[i] = y[i] - low[i][k] * y[k]
    for i in range(5, -1, -1):
        q[i] = y[i] / D[i]
        for k in range(i + 1, 6):
            q[i] = q[i] - low[k][i] * q[k]
    out = []
    for k in range(nj):
        acc = rows[0][k] * q[0] + rows[1][k] * q[1]
        if k > 0:
            acc = acc + rows[2][k] * q[2]
        for r in (3, 4, 5):
            acc = acc + rows[r][k] * q[r]
        out.append(acc)
    return out


def _pose_limited_step(J, W, e, w, lam2, th, lo, hi, limited):
    """pose_step on every row: _limited_step with _pose_solve."""
    n, nj = th.shape
    lock = np.zeros((n, nj), bool)
    resolves = np.zeros(n, np.int32)
    while True:
        d = _pose_solve(J, W, e, w, lam2, lock)
        dd = np.stack(d, axis=1)
        new = (((th <= lo) & (dd < 0)) | ((th >= hi) & (dd > 0))) & limited & ~lock
        lock = lock | new
        grew = new.any(axis=1)
        resolves = resolves + grew.astype(np.int32)
        if not grew.any():
            return d, lock, resolves


def _pose_attempt(consts, p, G, th, tol, rot_tol, w, max_iter, lam2, lo, hi, limited, dtype):
    """One attempt of every row from the placed angles th: (theta, steps, ep, er)."""
    n = p.shape[0]
    it = np.zeros(n, np.int32)
    ep, er = np.zeros(n, dtype), np.zeros(n, dtype)
    active = np.ones(n, bool)
    while n:
        s, c = np.sin(th), np.cos(th)
        (x, y, z), J = _chain_cs(consts, s, c)
        r, W = _pose_frame_cs(consts, s, c)
        ex, ey, ez = p[:, 0] - x, p[:, 1] - y, p[:, 2] - z
        en = np.sqrt(ex * ex + ey * ey + ez * ez)
        rn = _rot_error(r, G)
        if consts[4]:
            en = rn = np.full(n, np.nan, dtype)
        ep, er = np.where(active, en, ep), np.where(active, rn, er)
        above = (ep > tol) | (er > rot_tol)
        active = active & ~(~above | np.isnan(ep) | np.isnan(er) | (it == max_iter))
        if not active.any():
            break
        e = [ex, ey, ez] + [w * v for v in _rot_step_error(r, G)]
        if limited.any():
            d, _, _ = _pose_limited_step(J, W, e, w, lam2, th, lo, hi, limited)
        else:
            d = _pose_solve(J, W, e, w, lam2, None)
        th = np.where(active[:, None], _update(th, d, lo, hi, limited, dtype), th)
        it = it + active.astype(np.int32)
    return th, it, ep, er


def chain_fk_pose(dh, ang):
    """The tool pose of the DH chain at ang (n x nj or nj) through the restatement's
    chain: (p n x 3, R n x 3 x 3) float64, what ik_fk_chain's last transform holds."""
    dh = np.asarray(dh, np.float64)
    th = np.asarray(ang, np.float64).reshape(-1, dh.shape[1])
    consts = _consts(dh, np.float64)
    s, c = np.sin(th), np.cos(th)
    (x, y, z), _ = _chain_cs(consts, s, c)
    r, _ = _pose_frame_cs(consts, s, c)
    R = np.stack([np.stack(col, axis=1) for col in r], axis=2)
    return np.stack([x, y, z], axis=1), R


def check_pose_weights(rot_tol, rot_weight):
    """The library's refusals of rot_tol and rot_weight."""
    if np.isnan(rot_tol):
        raise ValueError("rot_tol must be a number")
    if not (np.isfinite(rot_weight) and rot_weight >= 0):
        raise ValueError("rot_weight must be finite and >= 0")


def chain_pose_reference(pts, rot, seed, tol=DEFAULT_TOL, rot_tol=None, rot_weight=1.0,
                         max_iter=DEFAULT_MAX_ITER, damping=DEFAULT_DAMPING, dh=None,
                         joint_limits=None, restarts=0, dtype=np.float64):
    """ik_chain_pose_solve of every (pts[i], rot[i], seed[i]) on the DH table dh (4 x nj),
    operation for operation; rot n x 3 x 3 or n x 9, rot_tol None: tol; seed None: the
    table's theta row.  Returns (theta n x nj, iters, tries, ep, er) in dtype."""
    dh = chain_dh(dh)
    nj = dh.shape[1]
    check_steps(max_iter, restarts)
    rot_tol = tol if rot_tol is None else rot_tol
    check_pose_weights(rot_tol, rot_weight)
    dtype = np.dtype(dtype).type
    consts = _consts(dh, dtype)
    p = np.asarray(pts, dtype).reshape(-1, 3)
    G = np.asarray(rot, dtype).reshape(-1, 9)
    n = p.shape[0]
    if G.shape[0] != n:
        raise ValueError(f"rot: {G.shape[0]} rotations for {n} points")
    lo64, hi64 = chain_limit_arrays(joint_limits, nj)
    limited = ~((lo64 == -np.inf) & (hi64 == np.inf))
    lo, hi = lo64.astype(dtype), hi64.astype(dtype)
    if seed is None:
        seed = np.tile(dh[0], (n, 1))
    tol, rot_tol, w = dtype(tol), dtype(rot_tol), dtype(rot_weight)
    lam2 = dtype(np.float64(damping) * np.float64(damping))
    pi = dtype(np.float64(3.141592653589793))
    slo, shi = np.where(limited, lo, -pi), np.where(limited, hi, pi)
    with np.errstate(all="ignore"):
        th0 = _place(np.asarray(seed, dtype).reshape(-1, nj), lo, hi, limited, dtype)
        best_th, tot, best_ep, best_er = _pose_attempt(consts, p, G, th0, tol, rot_tol, w,
                                                       max_iter, lam2, lo, hi, limited, dtype)
        best_score = best_ep + w * best_er
        tries = np.zeros(n, np.int32)
        last_ep, last_er = best_ep, best_er
        rows = np.arange(n)
        for a in range(1, int(restarts) + 1):
            # (a NaN error does not restart)
            keep = ((last_ep > tol) | (last_er > rot_tol)) & ~(np.isnan(last_ep) | np.isnan(last_er))
            rows = rows[keep]
            if rows.size == 0:
                break
            u = np.stack([start_u(rows, a, j) for j in range(nj)], axis=1).astype(dtype)
            start = _place(slo + u * (shi - slo), lo, hi, limited, dtype)
            th, it, last_ep, last_er = _pose_attempt(consts, p[rows], G[rows], start, tol, rot_tol,
                                                     w, max_iter, lam2, lo, hi, limited, dtype)
            tot[rows] += it
            score = last_ep + w * last_er
            better = score < best_score[rows]
            k = rows[better]
            best_th[k], best_ep[k], best_er[k] = th[better], last_ep[better], last_er[better]
            best_score[k], tries[k] = score[better], a
    return best_th, tot, tries, best_ep, best_er


def as_poses(poses):
    """(points n x 3, rotations n x 9) float64 from n x 4 x 4 transforms or a pair
    (points n x 3, rotations n x 3 x 3)."""
    if isinstance(poses, (tuple, list)) and len(poses) == 2 and np.ndim(poses[0]) == 2 \
            and np.shape(poses[0])[1] == 3:
        p = np.array(poses[0], np.float64)
        G = np.array(poses[1], np.float64)
        if G.shape != (p.shape[0], 3, 3):
            raise ValueError(f"poses: rotations of shape {G.shape} for {p.shape[0]} points, "
                             "expected n x 3 x 3")
        return p, G.reshape(-1, 9)
    M = np.asarray(poses, np.float64)
    if M.size == 0:
        return np.zeros((0, 3)), np.zeros((0, 9))
    if M.ndim != 3 or M.shape[1:] != (4, 4):
        raise ValueError("poses must be n x 4 x 4 transforms or a pair (points n x 3, rotations "
                         "n x 3 x 3)")
    return np.ascontiguousarray(M[:, :3, 3]), np.ascontiguousarray(M[:, :3, :3]).reshape(-1, 9)


class ChainInverseKinematics:
    """Inverse kinematics of a DH chain of 2..8 revolute joints on the GPU (libikhip
    ik_chain_solve): damped least squares inside per-joint limits, restarted from
    uniform points when an attempt ends above tol.  dh_matrix: rows theta, d, a,
    alpha, nj columns; the theta row is the home pose that seeds a solve without
    seeds.  joint_limits: what chain_limit_arrays takes.  strict: ikine raises
    OutOfRobotReachException for the lowest row that ends above tol.  ikine_pose
    (ik_chain_pose_solve) takes tool poses: rot_tol (None: tol) bounds the chord
    sqrt(1/2 |R - G|_F^2) of a converged row, rot_weight weighs the rotation rows of
    the step against the position rows (radians against the table's length unit)."""

    def __init__(self, dh_matrix, joint_limits=None, tol=DEFAULT_TOL, max_iter=DEFAULT_MAX_ITER,
                 damping=DEFAULT_DAMPING, restarts=DEFAULT_RESTARTS, strict=True, rot_tol=None,
                 rot_weight=1.0):
        self.dh_matrix = chain_dh(dh_matrix)
        self.nj = self.dh_matrix.shape[1]
        lo, hi = chain_limit_arrays(joint_limits, self.nj)
        free = bool((np.isneginf(lo) & np.isposinf(hi)).all())
        self.joint_limits = None if free else (lo, hi)
        check_steps(max_iter, restarts)
        if np.isnan(tol) or not (np.isfinite(damping) and damping > 0):
            raise ValueError("tol must be a number, damping finite and > 0")
        self.tol, self.max_iter, self.damping = float(tol), int(max_iter), float(damping)
        self.restarts, self.strict = int(restarts), bool(strict)
        self.rot_tol = self.tol if rot_tol is None else float(rot_tol)
        self.rot_weight = float(rot_weight)
        check_pose_weights(self.rot_tol, self.rot_weight)
        self.last_iters = self.last_tries = self.last_fk_err = self.last_stats = None
        self.last_rot_err = None

    def ikine(self, dest_points, seed=None):
        """Joint angles [theta1..theta_nj] (float64) for every destination point;
        seed (n x nj) starts attempt 0 of every row instead of the home pose."""
        from .. import _native
        from ..robot.robot import OutOfRobotReachException
        from .inverse import as_points
        pts = as_points(dest_points)
        if pts.shape[0] == 0:
            return []
        ang, it, tries, err, st = _native.context().chain_solve(
            self.dh_matrix, pts, seed, self.joint_limits, self.tol, self.max_iter, self.damping,
            self.restarts)
        self.last_iters, self.last_tries, self.last_fk_err, self.last_stats = it, tries, err, st
        if self.strict and st.first_err >= 0:
            i = st.first_err
            raise OutOfRobotReachException(
                f'Inverse Kinematics exception, point {dest_points[i]} not reached: '
                f'|FK(theta) - p| = {err[i]:.6g} > {self.tol:g} after {int(it[i])} steps')
        return ang.tolist()

    def ikine_pose(self, poses, seed=None):
        """Joint angles for every tool pose: poses n x 4 x 4 (what fkine returns last,
        ik_fk_chain's last transform) or a pair (points n x 3, rotations n x 3 x 3)."""
        from .. import _native
        from ..robot.robot import OutOfRobotReachException
        pts, rot = as_poses(poses)
        if pts.shape[0] == 0:
            return []
        ang, it, tries, err, rerr, st = _native.context().chain_pose_solve(
            self.dh_matrix, pts, rot, seed, self.joint_limits, self.tol, self.rot_tol,
            self.rot_weight, self.max_iter, self.damping, self.restarts)
        self.last_iters, self.last_tries, self.last_fk_err, self.last_stats = it, tries, err, st
        self.last_rot_err = rerr
        if self.strict and st.first_err >= 0:
            i = st.first_err
            raise OutOfRobotReachException(
                f'Inverse Kinematics exception, pose at {pts[i].tolist()} not reached: '
                f'|FK(theta) - p| = {err[i]:.6g} (tol {self.tol:g}), rotation error = '
                f'{rerr[i]:.6g} (tol {self.rot_tol:g}) after {int(it[i])} steps')
        return ang.tolist()
