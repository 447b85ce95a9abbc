"""python -m inversekinematicsann_amd.train -- train the ANN solver on the GPU.

Generates positions with position_generator.random_dist, labels them with the
GPU FABRIK solver (tol 1e-5, 200 iterations; rows whose solve raised are
dropped), fits the reference's network with ANN.fit (kinematics/ann.py:27-68),
saves it as `<prefix>_<timestamp>.h5` + scalers and prints the FK error of its
predictions on the held-out part.
"""
from __future__ import annotations

import argparse
import json
import time

import numpy as np


def label_positions(ctx, pts, tol=1e-5, max_iter=200):
    """(positions, angles) of the rows FABRIK solved: the reference raises on the
    first point outside the workspace or whose angles fail (inverse.py:26-35,
    54-112); a training set simply leaves such rows out."""
    from .robot.robot import SixDOFRobot
    lim = SixDOFRobot.effector_workspace_limits
    lo = np.array([lim[k][0] for k in ("x", "y", "z")], np.float64)
    hi = np.array([lim[k][1] for k in ("x", "y", "z")], np.float64)
    pts = pts[((pts >= lo) & (pts <= hi)).all(axis=1)]
    # a point whose solve raised has fk_err NaN (ik_fabrik_solve_fk)
    ang, _, err, _ = ctx.fabrik_solve_fk(pts, tol, max_iter, check_limits=False)
    ok = np.isfinite(err) & np.isfinite(ang).all(axis=1)
    return pts[ok], ang[ok]


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m inversekinematicsann_amd.train",
                                 description=__doc__.split("\n\n")[0])
    ap.add_argument("--samples", type=int, required=True, help="positions to generate")
    ap.add_argument("--epochs", type=int, required=True)
    ap.add_argument("--prefix", required=True, help="model file prefix (ANN.save_model)")
    ap.add_argument("--hidden", default="12,500", help="hidden layers as COUNT,UNITS (tanh)")
    ap.add_argument("--lr", type=float, default=1e-5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--patience", type=int, default=12)
    ap.add_argument("--mse-weight", type=float, default=1.0,
                    help="weight of the mean squared error of the scaled angles")
    ap.add_argument("--fk-weight", type=float, default=0.0,
                    help="weight of the mean squared |FK(theta) - p| of the network's angles")
    args = ap.parse_args(argv)
    count, units = (int(v) for v in args.hidden.split(","))

    from . import _native
    from .kinematics.ann import ANN
    from .kinematics.train import split_indices
    from .robot.position_generator import random_dist
    from .robot.robot import SixDOFRobot

    ctx = _native.context()
    pts, ang = label_positions(ctx, random_dist(args.samples, seed=args.seed))
    print(f"{len(pts)} of {args.samples} positions labelled by FABRIK (tol 1e-5 / 200)")
    ann = ANN(SixDOFRobot.effector_workspace_limits, SixDOFRobot.dh_matrix)
    t0 = time.perf_counter()
    hist = ann.fit(args.epochs, pts, ang, batch_size=args.batch, learning_rate=args.lr,
                   patience=args.patience, hidden=(count, units, "tanh"), seed=args.seed,
                   verbose=True, mse_weight=args.mse_weight, fk_weight=args.fk_weight)
    secs = time.perf_counter() - t0
    path = ann.save_model(args.prefix)
    _, held = split_indices(len(pts))
    _, err, _ = ann.predict_with_fk_error(pts[held])
    out = {"model": path, "epochs_run": len(hist["loss"]),
           "best_epoch": hist["best_epoch"], "stopped_epoch": hist["stopped_epoch"],
           "loss": hist["loss"][-1], "val_loss": hist["val_loss"],
           "fit_seconds": round(secs, 3), "held_out": int(len(held)),
           "fk_err_mean_m": float(np.nanmean(err)),
           "fk_err_max_m": float(np.nanmax(err))}
    if args.fk_weight > 0:
        out["fk"], out["val_fk"] = hist["fk"][-1], hist["val_fk"]
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
