"""Training-step time of the reference network (Input(3), 12 x Dense(500, tanh),
Dense(4); csrc/ik_train.hip) at batch 32 and batch 1024, against a torch eager
step of the same network on the same GPU in the same process (torch.nn.Linear /
tanh / mse_loss / torch.optim.Adam(eps=1e-7)).

Per batch size: the median of `steps` steps after `warmup`, each step timed on the
host around a blocking ik_ann_train_step (one H2D copy of the batch, the step's
kernels, one D2H copy of the loss) and around a torch step that ends in
loss.item(); the kernels of one step and their summed HIP-event time come from
ik_kernel_times.  With --epoch also the per-step time inside ik_ann_train_epoch
(no host round trip between steps).  One JSON line per batch size and loss.

--fk-weight W[,W2...] times the step under loss = mse + W * fk (ik_ann_train_set_loss
with the reference model's scalers; 0 = the plain mse path) for every W of the list in
this one process, so that the forward-kinematics term is compared with the plain loss
from the same build on the same visit.  The torch step is the plain mse one.

    python tools/train_bench.py [--steps 200] [--warmup 20] [--batches 32,1024] [--epoch]
                                [--fk-weight 0,1]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

DIMS = (3,) + (500,) * 12 + (4,)


def torch_step_ms(m, x, y, lr, steps, warmup):
    import torch
    layers = []
    for i, (w, b) in enumerate(zip(m.weights, m.biases)):
        lin = torch.nn.Linear(w.shape[0], w.shape[1])
        with torch.no_grad():
            lin.weight.copy_(torch.from_numpy(w.T))
            lin.bias.copy_(torch.from_numpy(b))
        layers.append(lin)
        if i < len(m.weights) - 1:
            layers.append(torch.nn.Tanh())
    net = torch.nn.Sequential(*layers).cuda()
    opt = torch.optim.Adam(net.parameters(), lr=lr, eps=1e-7)
    ts = []
    for i in range(warmup + steps):
        t0 = time.perf_counter()
        xb = torch.from_numpy(x).cuda()
        yb = torch.from_numpy(y).cuda()
        opt.zero_grad(set_to_none=True)
        loss = torch.nn.functional.mse_loss(net(xb), yb)
        loss.backward()
        opt.step()
        loss.item()
        if i >= warmup:
            ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batches", default="32,1024")
    ap.add_argument("--epoch", action="store_true")
    ap.add_argument("--fk-weight", default="0", help="weights of the fk term, comma-separated")
    args = ap.parse_args()
    from inversekinematicsann_amd import _native
    from inversekinematicsann_amd.kinematics.ann import (REFERENCE_X_SCALER, REFERENCE_Y_SCALER,
                                                         glorot_model)
    ctx = _native.Context(0)
    m = glorot_model(DIMS, seed=0)
    rng = np.random.default_rng(0)
    for batch in (int(b) for b in args.batches.split(",")):
        x = rng.standard_normal((batch, 3)).astype(np.float32)
        y = rng.standard_normal((batch, 4)).astype(np.float32)
        torch_ms = None
        for fkw in (float(w) for w in args.fk_weight.split(",")):
            ctx.train_begin(m.weights, m.biases, m.activations, max_batch=batch, lr=1e-5)
            if fkw > 0:
                ctx.train_set_loss(1.0, fkw, (REFERENCE_X_SCALER.mean, REFERENCE_X_SCALER.scale),
                                   (REFERENCE_Y_SCALER.mean, REFERENCE_Y_SCALER.scale))
            ts = []
            for i in range(args.warmup + args.steps):
                t0 = time.perf_counter()
                ctx.train_step(x, y)
                if i >= args.warmup:
                    ts.append((time.perf_counter() - t0) * 1e3)
            ctx.set_timing(True)
            ctx.train_step(x, y)
            ks = ctx.kernel_times()
            ctx.set_timing(False)
            out = {"batch": batch, "fk_weight": fkw, "ms_per_step": statistics.median(ts),
                   "kernels_per_step": len(ks), "kernel_ms_events": sum(v for _, v in ks)}
            by = {}
            for k, v in ks:
                by[k] = by.get(k, 0.0) + v
            out["kernel_ms_by_name"] = {k: round(v, 4) for k, v in by.items()}
            if args.epoch:
                n = batch * 64
                xe = rng.standard_normal((n, 3)).astype(np.float32)
                ye = rng.standard_normal((n, 4)).astype(np.float32)
                ctx.train_data(xe, ye)
                ctx.train_epoch(None, batch)
                t0 = time.perf_counter()
                ctx.train_epoch(None, batch)
                out["ms_per_step_in_epoch"] = (time.perf_counter() - t0) * 1e3 / 64
            ctx.train_end()
            if torch_ms is None:
                torch_ms = torch_step_ms(m, x, y, 1e-5, args.steps, args.warmup)
            out["torch_eager_ms_per_step"] = torch_ms
            out["torch_over_ikhip"] = out["torch_eager_ms_per_step"] / out["ms_per_step"]
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
