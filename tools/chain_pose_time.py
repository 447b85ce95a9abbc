#!/usr/bin/env python3
"""Kernel times of ik_chain_pose_solve (DESIGN.md section 3 "Chain pose solve"),
dispatch-stamped (ik_ctx_set_timing), device pointers, n rows (default 1M), at nj = 6 and
7 on tests/chain_fixtures.py's tables: pose goals (p, G) = FK(theta*), seeds 0.05 rad off,
tol = rot_tol, against ik_chain_solve on the same tables, seeds and position goals, the
two calls interleaved run by run.  The two solve different problems and take different
steps, so the mean step counts stand beside the times.

Every figure is the median of --runs timed calls after --warmup, with min and max.
Prints one JSON object (and writes it to --out).

    python tools/chain_pose_time.py [--n 1000000] [--runs 10] [--warmup 3] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.chain_time import spread, utilisation  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tol", type=float, default=1e-6)
    ap.add_argument("--max-iter", type=int, default=30)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    import torch
    from inversekinematicsann_amd import _native as N
    from inversekinematicsann_amd.kinematics.chain import chain_fk_pose
    from tests.chain_fixtures import table
    ctx = N.Context(0)
    n = a.n
    flags = N.IK_F_DEVICE
    ctx.set_timing(True)
    out = {"n": n, "tol": a.tol, "max_iter": a.max_iter}

    def one(call, kernel):
        st = call()
        ms = [t for k, t in ctx.kernel_times() if k == kernel]
        assert len(ms) == 1, ctx.kernel_times()
        return ms[0], st

    def leg(di, st, ms):
        it = di.cpu().numpy()
        return {"kernel": spread(ms), "mean_iters": float(it.mean()), "max_iters": int(it.max()),
                "n_capped": int(st.n_capped), "lane_utilisation": utilisation(it)}

    for nj in (6, 7):
        dh = table(nj)
        rng = np.random.default_rng(300 + nj)
        th = rng.uniform(-np.pi / 2, np.pi / 2, (n, nj))
        p, R = chain_fk_pose(dh, th)
        dp, dg = torch.from_numpy(p).cuda(), torch.from_numpy(R.reshape(n, 9).copy()).cuda()
        ds = torch.from_numpy(th + rng.normal(0, 0.05, (n, nj))).cuda()
        da = torch.empty((n, nj), dtype=torch.float64, device="cuda")
        di, dt = (torch.empty((n,), dtype=torch.int32, device="cuda") for _ in range(2))
        de, dr = (torch.empty((n,), dtype=torch.float64, device="cuda") for _ in range(2))
        di2 = torch.empty_like(di)
        c_ms, p_ms = [], []
        for r in range(a.warmup + a.runs):
            mc, sc = one(lambda: ctx.chain_solve_device(dh, dp, da, ds, di2, dt, de, None, a.tol,
                                                        a.max_iter, 1e-3, 0, flags),
                         "chain_solve_kernel")
            mp, sp = one(lambda: ctx.chain_pose_solve_device(dh, dp, dg, da, ds, di, dt, de, dr, None,
                                                             a.tol, a.tol, 1.0, a.max_iter, 1e-3, 0,
                                                             flags), "chain_pose_kernel")
            if r >= a.warmup:
                c_ms.append(mc)
                p_ms.append(mp)
        position, pose = leg(di2, sc, c_ms), leg(di, sp, p_ms)
        out[f"nj{nj}"] = {
            "position": position, "pose": pose,
            "ratio_of_medians": float(np.median(p_ms) / np.median(c_ms)),
            "ratio_per_step": float(np.median(p_ms) / np.median(c_ms)
                                    * position["mean_iters"] / pose["mean_iters"]),
            "max_rot_err_converged": float(dr[(de <= a.tol) & (dr <= a.tol)].max().item())}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
