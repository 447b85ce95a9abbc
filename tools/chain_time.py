#!/usr/bin/env python3
"""Kernel times of ik_chain_solve (DESIGN.md section 3 "Chain solve"), dispatch-stamped
(ik_ctx_set_timing), device pointers, n rows (default 1M):

  nj4        the refine fixture's distribution (tools/refine_time.py): ik_chain_solve at
             nj = 4, restarts 0, against ik_refine on the same rows, the two calls
             interleaved run by run; free, and under limits that never bind (the limited
             instantiations); the angles are checked bit-equal;
  nj6, nj8   tests/chain_fixtures.py's tables: goals FK(theta*), seeds 0.05 rad off;
  home6      the 6-joint table from its home pose, --home-iter steps an attempt, with
             0 and --restarts restarts: time, capped rows, lane utilisation.

Every figure is the median of --runs timed calls after --warmup, with min and max.
Prints one JSON object (and writes it to --out).

    python tools/chain_time.py [--n 1000000] [--runs 10] [--warmup 3] [--out FILE]
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


def utilisation(it):
    it = it.astype(np.int64)
    waves = np.concatenate([it, np.zeros((-len(it)) % 64, np.int64)]).reshape(-1, 64)
    return float(it.sum() / max(1, 64 * waves.max(axis=1).sum()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tol", type=float, default=1e-6)
    ap.add_argument("--max-iter", type=int, default=20)
    ap.add_argument("--home-iter", type=int, default=15)
    ap.add_argument("--restarts", type=int, default=3)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    import torch
    from inversekinematicsann_amd import _native as N
    from inversekinematicsann_amd.kinematics.chain import chain_fk
    from inversekinematicsann_amd.robot.robot import SixDOFRobot
    from tests.chain_fixtures import table
    ctx = N.Context(0)
    n = a.n
    flags = N.IK_F_DEVICE | N.IK_F_NO_LIMITS
    ctx.set_timing(True)
    out = {"n": n, "tol": a.tol, "max_iter": a.max_iter}

    def buffers(nj):
        return (torch.empty((n, nj), dtype=torch.float64, device="cuda"),
                torch.empty((n,), dtype=torch.int32, device="cuda"),
                torch.empty((n,), dtype=torch.int32, device="cuda"),
                torch.empty((n,), dtype=torch.float64, device="cuda"))

    def one(call, kernel):
        st = call()
        ms = [t for k, t in ctx.kernel_times() if k == kernel]
        assert len(ms) == 1, ctx.kernel_times()
        return ms[0], st

    def leg(di, st, ms):
        it = di.cpu().numpy()
        return {"kernel": spread(ms), "mean_iters": float(it.mean()), "max_iters": int(it.max()),
                "n_capped": int(st.n_capped), "lane_utilisation": utilisation(it)}

    # -- nj = 4 against refine_kernel, interleaved
    rng = np.random.default_rng(7)
    th = np.stack([rng.uniform(-np.pi / 2, np.pi / 2, n), rng.uniform(0, np.pi / 2, n),
                   rng.uniform(-np.pi / 2, 0, n), rng.uniform(-np.pi / 2, np.pi / 2, n)], axis=1)
    dh4 = np.asarray(SixDOFRobot.dh_matrix, np.float64)
    pts = ctx.fk(th)[0]
    dp = torch.from_numpy(pts).cuda()
    ds = torch.from_numpy(th + rng.normal(0, 0.05, (n, 4))).cuda()
    da, di, dt, de = buffers(4)
    da2 = torch.empty_like(da)
    pi4 = (np.full(4, -np.pi), np.full(4, np.pi))
    for name, lim, kr, kc in (("nj4_free", None, "refine_kernel", "chain_solve_kernel"),
                              ("nj4_never_binding", pi4, "refine_limited_kernel",
                               "chain_solve_limited_kernel")):
        ctx.set_joint_limits(lim)
        r_ms, c_ms = [], []
        for r in range(a.warmup + a.runs):
            mr, sr = one(lambda: ctx.refine_device(dp, ds, da2, di, de, tol=a.tol,
                                                   max_iter=a.max_iter, flags=flags), kr)
            mc, sc = one(lambda: ctx.chain_solve_device(dh4, dp, da, ds, di, dt, de, lim, a.tol,
                                                        a.max_iter, 1e-3, 0, flags), kc)
            if r >= a.warmup:
                r_ms.append(mr)
                c_ms.append(mc)
        out[name] = {"refine": spread(r_ms), "chain": leg(di, sc, c_ms),
                     "ratio_of_medians": float(np.median(c_ms) / np.median(r_ms)),
                     "bit_equal": bool(torch.equal(da, da2))}
    ctx.set_joint_limits(None)

    # -- nj = 6, 8: seeds 0.05 rad off
    for nj in (6, 8):
        dh = table(nj)
        rng = np.random.default_rng(100 + nj)
        th = rng.uniform(-np.pi / 2, np.pi / 2, (n, nj))
        dp = torch.from_numpy(chain_fk(dh, th)).cuda()
        ds = torch.from_numpy(th + rng.normal(0, 0.05, (n, nj))).cuda()
        da, di, dt, de = buffers(nj)
        ms = []
        for r in range(a.warmup + a.runs):
            m, st = one(lambda: ctx.chain_solve_device(dh, dp, da, ds, di, dt, de, None, a.tol,
                                                       a.max_iter, 1e-3, 0, flags),
                        "chain_solve_kernel")
            if r >= a.warmup:
                ms.append(m)
        out[f"nj{nj}"] = leg(di, st, ms)
        if nj == 6:  # -- and from the home pose, without and with restarts
            rng = np.random.default_rng(206)
            dp = torch.from_numpy(chain_fk(dh, rng.uniform(-np.pi, np.pi, (n, nj)))).cuda()
            for restarts in (0, a.restarts):
                ms = []
                for r in range(a.warmup + a.runs):
                    m, st = one(lambda: ctx.chain_solve_device(dh, dp, da, None, di, dt, de, None,
                                                               a.tol, a.home_iter, 1e-3, restarts,
                                                               flags), "chain_solve_kernel")
                    if r >= a.warmup:
                        ms.append(m)
                out[f"home6_restarts{restarts}"] = dict(
                    leg(di, st, ms), home_iter=a.home_iter,
                    attempts_returned=np.bincount(dt.cpu().numpy(), minlength=restarts + 1).tolist())
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
