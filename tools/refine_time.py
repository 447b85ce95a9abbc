#!/usr/bin/env python3
"""Kernel times of the damped-least-squares refine (DESIGN.md section 3 "Refine").

On n points (default 1M; the recipe of tests/test_refine_cpu.py's fixture: theta*
uniform in the robot's usual quadrant, goals FK(theta*) from the library's own FK,
seeds theta* + N(0, 0.05)) with ik_ctx_set_timing on, device pointers:

  refine      ik_refine at --tol: the refine kernel's time per call, the iteration
              counts and the lane utilisation sum_iters / sum over waves (64 x the
              wave's largest count), from the returned counts;
  limits      the same call under joint limits (ik_set_joint_limits), the limited
              kernel: with (-pi, pi) on every joint, limits that never bind, so only
              the cost of the variant shows (its angles are checked bit-equal to the
              free kernel's), and with the box the goals were drawn in -- [-pi/2, pi/2],
              [0, pi/2], [-pi/2, 0], [-pi/2, pi/2] -- with the rows that end on a limit
              and the rows the free kernel leaves outside (ik_check_joint_limits);
  fused       ik_ann_solve_refined with the 12 x 500 Glorot model: the ANN kernel's
              and the refine kernel's time (garbage seeds: the step cap decides);
  fabrik      ik_fabrik_solve_fk at 1e-5 / 200 on the same points.

Every figure is the median of --runs timed calls after --warmup, with min and max.
Prints one JSON object (and writes it to --out).

    python tools/refine_time.py [--n 1000000] [--runs 10] [--warmup 3] [--out FILE]
                                [--legs refine,limits,fused,fabrik]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def spread(v):
    v = np.asarray(v, np.float64)
    return {"median_ms": float(np.median(v)), "min_ms": float(v.min()), "max_ms": float(v.max()),
            "runs": int(v.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tol", type=float, default=1e-6)
    ap.add_argument("--max-iter", type=int, default=20)
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--legs", type=str, default="refine,limits,fused,fabrik")
    a = ap.parse_args()
    legs = set(a.legs.split(","))
    import torch
    from inversekinematicsann_amd import _native as N
    from inversekinematicsann_amd.kinematics.ann import (REFERENCE_X_SCALER, REFERENCE_Y_SCALER,
                                                         glorot_model)
    ctx = N.Context(0)
    n = a.n
    rng = np.random.default_rng(7)
    th = np.stack([rng.uniform(-np.pi / 2, np.pi / 2, n), rng.uniform(0, np.pi / 2, n),
                   rng.uniform(-np.pi / 2, 0, n), rng.uniform(-np.pi / 2, np.pi / 2, n)], axis=1)
    pts = ctx.fk(th)[0]
    seed = th + rng.normal(0, 0.05, (n, 4))
    dp, ds = torch.from_numpy(pts).cuda(), torch.from_numpy(seed).cuda()
    da = torch.empty((n, 4), dtype=torch.float64, device="cuda")
    di = torch.empty((n,), dtype=torch.int32, device="cuda")
    de = torch.empty((n,), dtype=torch.float64, device="cuda")
    flags = N.IK_F_DEVICE | N.IK_F_NO_LIMITS
    ctx.set_timing(True)

    def timed(call):
        """{kernel name: [ms per timed call]} and the last call's stats."""
        acc, st = {}, None
        for r in range(a.warmup + a.runs):
            st = call()
            if r < a.warmup:
                continue
            per = {}
            for name, ms in ctx.kernel_times():
                per[name] = per.get(name, 0.0) + ms
            for name, ms in per.items():
                acc.setdefault(name, []).append(ms)
            acc.setdefault("all", []).append(sum(per.values()))
        return acc, st

    out = {"n": n, "tol": a.tol, "max_iter": a.max_iter}

    def refine_leg(kernel):
        acc, st = timed(lambda: ctx.refine_device(dp, ds, da, di, de, tol=a.tol,
                                                  max_iter=a.max_iter, flags=flags))
        it = di.cpu().numpy().astype(np.int64)
        pad = np.zeros((-n) % 64, np.int64)
        waves = np.concatenate([it, pad]).reshape(-1, 64)
        return {"kernel": spread(acc[kernel]), "mean_iters": float(it.mean()),
                "max_iters": int(it.max()), "n_capped": int(st.n_capped),
                "max_fk_err": float(st.max_fk_err),
                "lane_utilisation": float(it.sum() / (64 * waves.max(axis=1).sum()))}

    # -- refine only
    if legs & {"refine", "limits"}:
        out["refine"] = refine_leg("refine_kernel")
    # -- the limited kernel: limits that never bind, then the goals' own box
    if "limits" in legs:
        free_ang = da.cpu().numpy()
        lo = np.array([-np.pi / 2, 0.0, -np.pi / 2, -np.pi / 2])
        hi = np.array([np.pi / 2, np.pi / 2, 0.0, np.pi / 2])
        ctx.set_joint_limits((np.full(4, -np.pi), np.full(4, np.pi)))
        out["refine_never_binding"] = refine_leg("refine_limited_kernel")
        out["refine_never_binding"]["bit_equal_to_free"] = bool(
            da.cpu().numpy().tobytes() == free_ang.tobytes())
        ctx.set_joint_limits((lo, hi))
        out["refine_limited"] = refine_leg("refine_limited_kernel")
        ang = da.cpu().numpy()
        out["refine_limited"].update(
            rows_on_a_limit=int(((ang == lo) | (ang == hi)).any(axis=1).sum()),
            rows_outside=int(ctx.check_joint_limits(da).n_capped),
            free_rows_outside=int(ctx.check_joint_limits(free_ang).n_capped))
        ctx.set_joint_limits(None)
    # -- the ANN's output as seeds, one call
    if "fused" in legs:
        m = glorot_model()
        ctx.ann_load(m.weights, m.biases, m.activations, REFERENCE_X_SCALER.mean,
                     REFERENCE_X_SCALER.scale, REFERENCE_Y_SCALER.mean, REFERENCE_Y_SCALER.scale)
        dse = torch.empty((n,), dtype=torch.float64, device="cuda")
        acc, st = timed(lambda: ctx.ann_solve_refined_device(dp, da, di, de, dse, tol=a.tol,
                                                             max_iter=a.max_iter, flags=flags))
        ref_ms = np.asarray(acc.pop("refine_kernel"))
        ann_ms = np.asarray(acc.pop("all")) - ref_ms
        out["fused"] = {"ann_kernels": sorted(acc), "ann": spread(ann_ms),
                        "refine": spread(ref_ms),
                        "refine_share": float(np.median(ref_ms / (ref_ms + ann_ms))),
                        "mean_iters": float(st.sum_iters / n), "n_capped": int(st.n_capped)}
    # -- FABRIK from its own seed pose
    if "fabrik" in legs:
        acc, st = timed(lambda: ctx.fabrik_solve_device(dp, da, di, None, tol=1e-5, max_iter=200,
                                                        flags=flags, fk_err=de))
        tot = acc.pop("all")
        out["fabrik_1e-5_200"] = {"kernels": sorted(acc), "all_kernels": spread(tot),
                                  "mean_iters": float(st.sum_iters / n),
                                  "max_iters": int(st.max_iters), "n_capped": int(st.n_capped),
                                  "max_fk_err": float(st.max_fk_err)}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
