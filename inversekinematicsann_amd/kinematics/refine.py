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
(the effector as Rz(t1) B1 Rz(t2) B2 Rz(t3) B3 Rz(t4) B4 e4 applied right to left,
B_i = Tz(d_i) Tx(a_i) Rx(alpha_i)), the same sums in the same order, no fused
multiply-add -- so in float64 it differs from the kernel only by the kernel's
sin / cos (within 1.2e-16 of libm's).

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
    angle rows th (n x 4): ik_refine.hip's sequence."""
    a, d, ca, sa, _ = consts
    s, c = np.sin(th), np.cos(th)
    n = th.shape[0]
    x = np.full(n, a[3], th.dtype)
    y = np.zeros(n, th.dtype)
    z = np.full(n, d[3], th.dtype)
    cols = []  # open columns, the latest joint first
    for i in (3, 2, 1, 0):
        ci, si = c[:, i], s[:, i]
        xr = ci * x - si * y
        yr = si * x + ci * y
        for w in cols:  # Rz(t_i) on the columns to its right
            wx = ci * w[0] - si * w[1]
            wy = si * w[0] + ci * w[1]
            w[0], w[1] = wx, wy
        cols.append([-yr, xr, np.zeros(n, th.dtype)])  # d Rz(t_i) v / dt_i
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


def refine_reference(pts, seed, tol=DEFAULT_TOL, max_iter=DEFAULT_MAX_ITER,
                     damping=DEFAULT_DAMPING, dh=None, dtype=np.float64):
    """The refine of every (pts[i], seed[i]); returns (theta n x 4, iters n int32,
    err n) in dtype (np.float64 or np.longdouble)."""
    if dh is None:
        from ..robot.robot import SixDOFRobot
        dh = SixDOFRobot.dh_matrix
    dtype = np.dtype(dtype).type
    consts = _consts(dh, dtype)
    p = np.asarray(pts, dtype).reshape(-1, 3)
    th = wrap(np.asarray(seed, dtype).reshape(-1, 4), dtype)
    n = p.shape[0]
    tol = dtype(tol)
    lam2 = dtype(np.float64(damping) * np.float64(damping))
    clamp = dtype(STEP_CLAMP)
    it = np.zeros(n, np.int32)
    err = np.zeros(n, dtype)
    active = np.ones(n, bool)
    with np.errstate(all="ignore"):
        while n:
            (x, y, z), (j0, j1, j2, j3) = _chain(consts, th)
            ex, ey, ez = p[:, 0] - x, p[:, 1] - y, p[:, 2] - z
            en = np.sqrt(ex * ex + ey * ey + ez * ez)
            if consts[4]:
                en = np.full(n, np.nan, dtype)
            err = np.where(active, en, err)
            active = active & ~(~(err > tol) | (it == max_iter))
            if not active.any():
                break
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
            m = np.fmax(np.fmax(np.abs(e0), np.abs(e1)), np.fmax(np.abs(e2), np.abs(e3)))
            big = m > clamp
            sc = np.where(big, clamp / np.where(big, m, 1), 1)
            d = np.stack([np.where(big, e * sc, e) for e in (e0, e1, e2, e3)], axis=1)
            th = np.where(active[:, None], wrap(th + d, dtype), th)
            it = it + active.astype(np.int32)
    return th, it, err
