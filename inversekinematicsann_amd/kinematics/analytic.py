"""The closed-form inverse kinematics of ik_analytic_solve, restated in numpy.

`analytic_reference` performs the row arithmetic of csrc/ik_analytic_row.h
(stated in include/ikhip.h "Analytic") operation for operation, in float64 or
np.longdouble; `planar_robot` is the acceptance rule of csrc/ik_analytic_plan.cpp.
Nothing here needs the native library: the module is what the kernel is tested
against and documents the method.
"""
from __future__ import annotations

import numpy as np

IK_ELBOW_UP, IK_ELBOW_DOWN = -1, 1
ELBOWS = {"up": IK_ELBOW_UP, "down": IK_ELBOW_DOWN}


def planar_robot(dh):
    """(d1, a1, a2, a3, a4) of a DH table (rows theta, d, a, alpha) that is a yaw
    joint followed by a planar three-link chain; ValueError naming the first entry
    that breaks the rule otherwise (the library's IK_E_BADARG)."""
    dh = np.asarray(dh, np.float64).reshape(4, 4)
    d, a, al = dh[1], dh[2], dh[3]
    if not abs(np.cos(al[0])) <= 1e-12 or not np.sin(al[0]) > 0.0:
        raise ValueError(f"alpha1 = {float(al[0])!r} must be +pi/2 (|cos| <= 1e-12, sin > 0)")
    for name, row, rule in (("alpha", al, "0"), ("d", d, "0")):
        for i in (1, 2, 3):
            if not row[i] == 0.0:
                raise ValueError(f"{name}{i + 1} = {float(row[i])!r} must be {rule}")
    for i in (1, 2, 3):
        if not np.isfinite(a[i]) or not a[i] > 0.0:
            raise ValueError(f"a{i + 1} = {float(a[i])!r} must be finite and > 0")
    if not np.isfinite(a[0]) or not a[0] >= 0.0:
        raise ValueError(f"a1 = {float(a[0])!r} must be finite and >= 0")
    return float(d[0]), float(a[0]), float(a[1]), float(a[2]), float(a[3])


def wrap(t, dtype=np.float64):
    """theta - 2 pi rint(theta / 2 pi) (ik_refine's wrap; 2 pi in the dtype)."""
    two_pi = dtype(2 * np.pi) if dtype is np.float64 else 8 * np.arctan(dtype(1))
    return t - two_pi * np.rint(t / two_pi)


def analytic_reference(pts, pitch, elbow, nearest, dh, dtype=np.float64):
    """(ang n x 4, pitch_used n, failed n bool, moved n bool) for goals pts, the
    pitches (None: every goal's own elevation gamma; a scalar or n values) and the
    elbow branch -1 / +1.  Failed rows are NaN in ang and pitch_used."""
    T = dtype
    d1, a1, a2, a3, a4 = (T(v) for v in planar_robot(dh))
    b = T(elbow)
    p = np.asarray(pts, T).reshape(-1, 3)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        t1 = np.arctan2(y, x)
        r = np.sqrt(x * x + y * y) - a1
        h = z - d1
        rho2 = r * r + h * h
        rho = np.sqrt(rho2)
        gam = np.arctan2(h, r)
        phi = gam.copy() if pitch is None else np.broadcast_to(np.asarray(pitch, T),
                                                               x.shape).copy()
        sa, da, k2 = a2 + a3, abs(a2 - a3), 2 * a2 * a3

        def wrist(phi):
            wr = r - a4 * np.cos(phi)
            wh = h - a4 * np.sin(phi)
            W = np.sqrt(wr * wr + wh * wh)
            return wr, wh, (sa - W) * (sa + W) / k2, (W - da) * (W + da) / k2

        wr, wh, m, q = wrist(phi)
        infeasible = ~((m >= 0) & (q >= 0))
        failed, moved = infeasible, np.zeros(len(p), bool)
        if nearest:
            den = 2 * a4 * rho
            cmin = (rho2 + a4 * a4 - sa * sa) / den
            cmax = (rho2 + a4 * a4 - da * da) / den
            dl = wrap(phi - gam, T)
            some = (cmin <= 1) & (cmax >= -1) & (rho > 0) & (dl == dl)
            lo = np.arccos(np.where(cmax < 1, cmax, T(1)))
            hi = np.arccos(np.where(cmin > -1, cmin, T(-1)))
            ad = np.abs(dl)
            ad = np.where(ad < lo, lo, ad)
            ad = np.where(ad > hi, hi, ad)
            moved = infeasible & some
            phi = np.where(moved, gam + np.where(dl < 0, T(-1), T(1)) * ad, phi)
            wr2, wh2, m2, q2 = wrist(phi)
            wr, wh = np.where(moved, wr2, wr), np.where(moved, wh2, wh)
            m = np.where(moved, np.where(m2 > 0, m2, T(0)), m)
            q = np.where(moved, np.where(q2 > 0, q2, T(0)), q)
            failed = infeasible & ~some
        s3 = b * np.sqrt(m * q)
        c3 = (q - m) / 2
        t3 = b * 2 * np.arctan2(np.sqrt(m), np.sqrt(q))
        t2 = np.arctan2(wh, wr) - np.arctan2(a3 * s3, a2 + a3 * c3)
        t4 = wrap(phi - t2 - t3, T)
        ang = np.stack([t1, wrap(t2, T), t3, t4], axis=1)
    ang[failed] = np.nan
    return ang, np.where(failed, T(np.nan), phi), failed, moved
