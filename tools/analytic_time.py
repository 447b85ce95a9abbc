#!/usr/bin/env python3
"""Kernel times of the closed-form solve (DESIGN.md section 3 "Analytic").

On n goals (default 1M; the recipe of tests/test_analytic_cpu.py's fixture A: theta*
with theta1 in (-pi/2, pi/2), theta2 / theta4 in (-pi, pi), theta3 = +-U(0.1, pi - 0.1),
goals FK(theta*) from the library's own FK, the rows with signed reach > 0.05), with
ik_ctx_set_timing on (dispatch-stamped kernel times), device pointers:

  strict      ik_analytic_solve at the rows' own pitch theta2 + theta3 + theta4;
  strict_random / nearest_random
              the same goals at pitches U(-pi, pi): a third or so infeasible, failed
              (strict) or moved (IK_F_PITCH_NEAREST);
  fabrik      ik_fabrik_solve_fk at 1e-5 / 200 on the same goals;
  refine      ik_refine (1e-6 / 20) from theta* + N(0, 0.05).

Every figure is the median of --runs timed calls after --warmup, with min and max;
hbm_floor_ms is the analytic call's bytes per row (24 + 8 in, 32 + 8 + 8 out) at
--hbm-gbs.  Prints one JSON object (and writes it to --out).

    python tools/analytic_time.py [--n 1000000] [--runs 10] [--warmup 3] [--out FILE]
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
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="HBM peak for the floor (GB/s)")
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    import torch
    from inversekinematicsann_amd import _native as N
    ctx = N.Context(0)
    n = a.n
    rng = np.random.default_rng(21)
    n3 = 3 * n
    sign = rng.choice([-1.0, 1.0], n3)
    th = np.stack([rng.uniform(-np.pi / 2, np.pi / 2, n3), rng.uniform(-np.pi, np.pi, n3),
                   sign * rng.uniform(0.1, np.pi - 0.1, n3), rng.uniform(-np.pi, np.pi, n3)],
                  axis=1)
    pts = ctx.fk(th)[0]
    reach = pts[:, 0] * np.cos(th[:, 0]) + pts[:, 1] * np.sin(th[:, 0])
    keep = np.flatnonzero(reach > 0.05)[:n]
    assert len(keep) == n
    pts, th = np.ascontiguousarray(pts[keep]), np.ascontiguousarray(th[keep])
    pitch = th[:, 1] + th[:, 2] + th[:, 3]
    pr = rng.uniform(-np.pi, np.pi, n)
    seed = th + rng.normal(0, 0.05, (n, 4))
    dp, dph, dpr = (torch.from_numpy(v).cuda() for v in (pts, pitch, pr))
    ds = torch.from_numpy(seed).cuda()
    da = torch.empty((n, 4), dtype=torch.float64, device="cuda")
    dpo = torch.empty((n,), dtype=torch.float64, device="cuda")
    de = torch.empty((n,), dtype=torch.float64, device="cuda")
    di = torch.empty((n,), dtype=torch.int32, device="cuda")
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

    floor_ms = n * (24 + 8 + 32 + 8 + 8) / (a.hbm_gbs * 1e9) * 1e3
    out = {"n": n, "hbm_gbs": a.hbm_gbs, "hbm_floor_ms": floor_ms}
    for name, ph, fl in (("strict", dph, flags), ("strict_random", dpr, flags),
                         ("nearest_random", dpr, flags | N.IK_F_PITCH_NEAREST)):
        acc, st = timed(lambda: ctx.analytic_solve_device(dp, da, ph, dpo, de, elbow=N.IK_ELBOW_UP,
                                                          flags=fl))
        k = spread(acc["analytic_kernel"])
        failed = int(torch.isnan(de).sum().item())
        out[name] = {"kernel": k, "hbm_fraction": floor_ms / k["median_ms"], "failed": failed,
                     "moved": int(st.n_capped), "max_fk_err": float(st.max_fk_err)}
    acc, st = timed(lambda: ctx.fabrik_solve_device(dp, da, di, None, tol=1e-5, max_iter=200,
                                                    flags=flags, fk_err=de))
    tot = acc.pop("all")
    out["fabrik_1e-5_200"] = {"kernels": sorted(acc), "all_kernels": spread(tot),
                              "mean_iters": float(st.sum_iters / n), "n_capped": int(st.n_capped),
                              "max_fk_err": float(st.max_fk_err)}
    acc, st = timed(lambda: ctx.refine_device(dp, ds, da, di, de, tol=1e-6, max_iter=20,
                                              flags=flags))
    out["refine_1e-6_20"] = {"kernel": spread(acc["refine_kernel"]),
                             "mean_iters": float(st.sum_iters / n), "n_capped": int(st.n_capped),
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
