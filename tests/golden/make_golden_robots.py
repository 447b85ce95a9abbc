"""Golden fixture for DH tables with no zero entry (tests/robots.py: GEN_A,
GEN_B, SKEW_DH), by importing the reference.

Run in the build container only (see make_golden.py for the keras stub and the
iteration counter; the reference never travels to the GPU box):

    python tests/golden/make_golden_robots.py

Writes tests/golden/robots_general_dh.npz.  Per table <T>:
  <T>_dh                  the table (rows theta, d, a, alpha)
  <T>_points              400 goals inside the default limits (the reference's
                          ikine checks them): a uniform box and the x >= 0 edge
                          rows of tests/robots.py (no NaN row: the reference's
                          limit check is not what this fixture pins)
  <T>_angles_<k>, _iters_<k>, _joints_<k>, _status_<k>
                          FabrikInverseKinematics.ikine point by point at
                          k = 0: tol 1e-3 / 100 iterations, k = 1: 1e-5 / 200;
                          status 0, 2 (ValueError), 3 (ZeroDivisionError) or 4
                          (OutOfRobotReachException of fkine); NaN / -1 where it raised
  <T>_fk_angles, _fk_mats 100 angle rows in [-2 pi, 2 pi] and the four cumulative
                          4 x 4 matrices of ForwardKinematics.fkine
Only inputs and the reference's outputs are saved.
"""
from __future__ import annotations

import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import robots as RB  # noqa: E402  (before the reference's own tests package is on the path)
import make_golden as MG  # noqa: E402  (imports the reference, stubs keras)

N_POINTS, N_FK = 400, 100
NAME = "robots_general_dh.npz"


def golden_points(dh):
    rng = np.random.default_rng(43)
    lo, hi = RB.DEFAULT_LIMITS[0::2], RB.DEFAULT_LIMITS[1::2]
    pts = rng.uniform(lo, hi, (N_POINTS, 3))
    e = RB.edge_goals(dh, x_sign=(1.0,))
    e = e[~np.isnan(e).any(axis=1)]
    pts[N_POINTS - len(e):] = e
    return pts


def ref_ikine(dh_table, points, tol, max_iter):
    """make_golden.ref_ikine_with_iters with the robot's table as an argument."""
    R = MG.R
    dh = [[float(v) for v in row] for row in dh_table]
    ik = MG.inverse.FabrikInverseKinematics(dh, R.links_lengths, R.effector_workspace_limits,
                                            tol, max_iter)
    fk = MG.forward.ForwardKinematics(dh)
    fab = MG.fabrik.Fabrik(R.links_lengths, tol, max_iter)
    nan4, nan43 = [np.nan] * 4, [[np.nan] * 3] * 4
    angles, iters, joints, status = [], [], [], []
    for p in points:
        try:
            MG._count["n"] = 0
            a = ik.ikine([list(p)])[0]
            it = MG._count["n"]
            # final joint positions: the same seed through Fabrik.calculate
            th = [math.atan2(p[1], p[0])] + dh[0][1:]
            _, fk_all = fk.fkine(th)
            init = [MG.inverse.Point([m[0][3], m[1][3], m[2][3]]) for m in fk_all]
            fin = fab.calculate(init, list(p))
            angles.append(a); iters.append(it); joints.append([list(q) for q in fin])
            status.append(0)
            continue
        except ZeroDivisionError:
            code = 3
        except ValueError:
            code = 2
        except MG.robot.OutOfRobotReachException:
            code = 4
        angles.append(nan4); iters.append(-1); joints.append(nan43); status.append(code)
    return (np.array(angles, np.float64), np.array(iters, np.int32),
            np.array(joints, np.float64), np.array(status, np.int32))


def main():
    out = {"tols": np.array([t for t, _ in RB.CONFIGS]),
           "max_iters": np.array([m for _, m in RB.CONFIGS], np.int32)}
    assert list(MG.R.links_lengths) == RB.LINKS.tolist()
    rng = np.random.default_rng(47)
    fk_ang = rng.uniform(-2 * math.pi, 2 * math.pi, (N_FK, 4))
    for name, dh in RB.TABLES.items():
        pts = golden_points(dh)
        out[f"{name}_dh"] = np.array(dh)
        out[f"{name}_points"] = pts
        for k, (tol, mi) in enumerate(RB.CONFIGS):
            a, it, jo, st = ref_ikine(dh, pts.tolist(), tol, mi)
            out.update({f"{name}_angles_{k}": a, f"{name}_iters_{k}": it,
                        f"{name}_joints_{k}": jo, f"{name}_status_{k}": st})
            print(f"{name} tol {tol:g}: mean iters {it[it >= 0].mean():.2f} "
                  f"capped {int((it == mi).sum())} errors {int((st != 0).sum())}")
        fk = MG.forward.ForwardKinematics([[float(v) for v in row] for row in dh])
        out[f"{name}_fk_angles"] = fk_ang
        out[f"{name}_fk_mats"] = np.array([[np.asarray(m, np.float64) for m in
                                            fk.fkine(list(a))[1]] for a in fk_ang])
    np.savez_compressed(os.path.join(HERE, NAME), **out)
    print(NAME, os.path.getsize(os.path.join(HERE, NAME)), "bytes")


if __name__ == "__main__":
    main()
