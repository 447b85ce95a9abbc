"""GPU training (ik_train.hip behind ik_ann_train_*): gradients, the Adam update,
a short training trajectory, determinism, ANN.fit end to end and misuse.

References are computed here on the CPU with torch: float64 autograd for the
gradients, a float64 restatement of Keras' Adam for the updates, and the same
trainer in float32 as the yardstick of what fp32 arithmetic costs.  Nothing is
pinned to Keras (it cannot run where these tests do).
"""
import math

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

FACTOR = 16.0  # GPU error <= FACTOR x the CPU-float32 error (MFMA order, exp2/rcp tanh vs libm)
B1, B2, EPS = 0.9, 0.999, 1e-7  # Keras' Adam defaults


@pytest.fixture(scope="module")
def ctx():
    from inversekinematicsann_amd import _native
    c = _native.Context(0)
    yield c
    c.close()


def _torch():
    import torch
    torch.set_num_threads(4)
    return torch


def _act(torch, name, z):
    return {"tanh": torch.tanh, "relu": torch.relu, "sigmoid": torch.sigmoid,
            "linear": lambda v: v}[name](z)


class CpuTrainer:
    """The trainer restated with torch on the CPU in `dtype`: forward, the loss
    sum((A_L - y)^2) / (rows n_out), autograd gradients, Keras' Adam."""

    def __init__(self, Ws, bs, acts, dtype, lr=1e-3):
        torch = _torch()
        self.torch, self.dtype, self.acts, self.lr = torch, dtype, list(acts), lr
        self.W = [torch.tensor(np.asarray(w, np.float64), dtype=dtype) for w in Ws]
        self.b = [torch.tensor(np.asarray(b, np.float64), dtype=dtype) for b in bs]
        self.m = [torch.zeros_like(p) for p in self.W + self.b]
        self.v = [torch.zeros_like(p) for p in self.W + self.b]
        self.t = 0

    def grads(self, x, y):
        torch = self.torch
        ps = [p.clone().requires_grad_(True) for p in self.W + self.b]
        n = len(self.W)
        h = torch.tensor(np.asarray(x, np.float64), dtype=self.dtype)
        yt = torch.tensor(np.asarray(y, np.float64), dtype=self.dtype)
        for l in range(n):
            h = _act(torch, self.acts[l], h @ ps[l] + ps[n + l])
        loss = ((h - yt) ** 2).sum() / (yt.shape[0] * yt.shape[1])
        loss.backward()
        return [p.grad for p in ps], float(loss.detach())

    def step(self, x, y):
        torch = self.torch
        g, loss = self.grads(x, y)
        self.t += 1
        alpha = self.lr * math.sqrt(1.0 - B2 ** self.t) / (1.0 - B1 ** self.t)
        ps = self.W + self.b
        with torch.no_grad():
            for i, p in enumerate(ps):
                self.m[i] = B1 * self.m[i] + (1.0 - B1) * g[i]
                self.v[i] = B2 * self.v[i] + (1.0 - B2) * g[i] * g[i]
                p -= alpha * self.m[i] / (torch.sqrt(self.v[i]) + EPS)
        return loss

    def epoch(self, x, y, perm, batch):
        tot = 0.0
        n = len(perm)
        for s in range(0, n, batch):
            idx = perm[s:s + batch]
            tot += self.step(x[idx], y[idx]) * len(idx)
        return tot / n


def _model(dims, seed, hidden_act="tanh"):
    from inversekinematicsann_amd.kinematics.ann import glorot_model
    m = glorot_model(tuple(dims), seed=seed, hidden_act=hidden_act)
    rng = np.random.default_rng(seed + 100)
    m.biases = [rng.uniform(-0.1, 0.1, b.shape).astype(np.float32) for b in m.biases]
    return m


def _batch(dims, rows, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((rows, dims[0])).astype(np.float32),
            rng.standard_normal((rows, dims[-1])).astype(np.float32))


def _rel(g, g64):
    g64 = np.asarray(g64, np.float64)
    return float(np.abs(np.asarray(g, np.float64) - g64).max() / np.abs(g64).max())


# ---- 1. gradients ------------------------------------------------------------
GRAD_CASES = [
    ((3, 40, 72, 4), 24, "tanh"),     # nothing a multiple of 32 or 8; less than one row tile
    ((3, 500, 500, 4), 32, "tanh"),   # the reference's widths
    ((3, 96, 64, 4), 160, "tanh"),    # several row tiles
    ((3, 33, 4), 1, "tanh"),          # single row
    ((5, 48, 48, 2), 40, "relu"),     # free input and output widths
    ((5, 48, 48, 2), 40, "sigmoid"),
    ((5, 48, 48, 2), 40, "linear"),
]


@pytest.mark.parametrize("dims,rows,act", GRAD_CASES,
                         ids=[f"{'x'.join(map(str, d))}-b{r}-{a}" for d, r, a in GRAD_CASES])
def test_gradients_match_float64_autograd(ctx, dims, rows, act):
    torch = _torch()
    m = _model(dims, seed=7, hidden_act=act)
    x, y = _batch(dims, rows, seed=8)
    ctx.train_begin(m.weights, m.biases, m.activations, max_batch=rows, lr=1e-3)
    try:
        gW, gb, loss = ctx.train_grads(x, y)
    finally:
        ctx.train_end()
    g64, loss64 = CpuTrainer(m.weights, m.biases, m.activations, torch.float64).grads(x, y)
    g32, _ = CpuTrainer(m.weights, m.biases, m.activations, torch.float32).grads(x, y)
    g64 = [g.numpy() for g in g64]
    yard = max(_rel(a.numpy(), b) for a, b in zip(g32, g64))
    errs = [_rel(a, b) for a, b in zip(gW + gb, g64)]
    print(f"grads {dims} b{rows} {act}: gpu worst {max(errs):.3e}, cpu-f32 yardstick "
          f"{yard:.3e}, ratio {max(errs) / yard:.2f}; loss {loss:.9g} vs {loss64:.9g}")
    assert abs(loss - loss64) <= 1e-5 * abs(loss64)
    for i, e in enumerate(errs):
        assert e <= FACTOR * yard, (i, e, yard)


# ---- 2. Adam -----------------------------------------------------------------
def test_adam_step_matches_float64_formulas(ctx):
    dims, rows, lr = (3, 40, 72, 4), 24, 1e-3
    m = _model(dims, seed=7)
    x, y = _batch(dims, rows, seed=8)
    ctx.train_begin(m.weights, m.biases, m.activations, max_batch=rows, lr=lr)
    try:
        def state():
            out = []
            for what in ("weights", "m", "v"):
                W, b = ctx.train_get(what)
                out.append([a.astype(np.float64) for a in W + b])
            return out
        for t in range(1, 4):
            w0, m0, v0 = state()
            gW, gb, _ = ctx.train_grads(x, y)
            ctx.train_step(x, y)
            w1, m1, v1 = state()
            alpha = lr * math.sqrt(1.0 - B2 ** t) / (1.0 - B1 ** t)
            for i, g in enumerate(gW + gb):
                g = g.astype(np.float64)
                me = B1 * m0[i] + (1.0 - B1) * g
                ve = B2 * v0[i] + (1.0 - B2) * g * g
                we = w0[i] - alpha * me / (np.sqrt(ve) + EPS)
                ulp_m = np.spacing(np.abs(me).astype(np.float32)).astype(np.float64)
                ulp_v = np.spacing(np.abs(ve).astype(np.float32)).astype(np.float64)
                dm, dv = np.abs(m1[i] - me) / ulp_m, np.abs(v1[i] - ve) / ulp_v
                dw = np.abs(w1[i] - we) - 2.0 ** -23 * np.abs(we)
                print(f"adam t={t} tensor {i}: m {dm.max():.2f} ulp, v {dv.max():.2f} ulp, "
                      f"W excess {dw.max() / alpha:.2e} alpha")
                assert dm.max() <= 4.0 and dv.max() <= 4.0
                assert (dw <= 1e-5 * alpha).all()
    finally:
        ctx.train_end()


# ---- 3. / 4. trajectory, determinism -------------------------------------------
TRAJ = [((3, 64, 64, 4), 32), ((3, 40, 72, 4), 24)]  # the second: a short last batch of 8
EPOCHS = 6


@pytest.fixture(scope="module")
def traj_data():
    from inversekinematicsann_amd.robot.position_generator import random_dist
    pts = random_dist(3072, seed=11)
    ang = O.fabrik_ikine(pts, 1e-3, 100)[0]
    pts, ang = pts[:2048], ang[:2048]
    x = ((pts - pts.mean(0)) / pts.std(0)).astype(np.float32)
    y = ((ang - ang.mean(0)) / ang.std(0)).astype(np.float32)
    return pts, ang, x, y


def _perms(n):
    rng = np.random.default_rng(0)
    return [rng.permutation(n).astype(np.int32) for _ in range(EPOCHS)]


def _gpu_traj(dims, batch, x, y):
    from inversekinematicsann_amd import _native
    from inversekinematicsann_amd.kinematics.ann import glorot_model
    m = glorot_model(tuple(dims), seed=3)
    c = _native.Context(0)
    try:
        c.train_begin(m.weights, m.biases, m.activations, max_batch=batch, lr=1e-3)
        c.train_data(x, y)
        losses = [c.train_epoch(p, batch)[0] for p in _perms(len(x))]
        W, b = c.train_get("weights")
        c.train_end()
    finally:
        c.close()
    return losses, W, b


@pytest.fixture(scope="module")
def traj_ref(traj_data):
    """Per case the float64 and float32 CPU trajectories (computed once)."""
    from inversekinematicsann_amd.kinematics.ann import glorot_model
    torch = _torch()
    _, _, x, y = traj_data
    out = []
    for dims, batch in TRAJ:
        m = glorot_model(tuple(dims), seed=3)
        row = {}
        for name, dt in (("f64", torch.float64), ("f32", torch.float32)):
            tr = CpuTrainer(m.weights, m.biases, m.activations, dt, lr=1e-3)
            row[name] = [tr.epoch(x, y, p, batch) for p in _perms(len(x))]
        out.append(row)
    return out


@pytest.fixture(scope="module")
def traj_gpu(traj_data):
    _, _, x, y = traj_data
    return [_gpu_traj(dims, batch, x, y) for dims, batch in TRAJ]


@pytest.mark.parametrize("case", [0, 1], ids=["3x64x64x4-b32", "3x40x72x4-b24"])
def test_trajectory_follows_float64(traj_ref, traj_gpu, case):
    f64 = [np.array(r["f64"]) for r in traj_ref]
    f32 = [np.array(r["f32"]) for r in traj_ref]
    yard = np.maximum(*[np.abs(a - b) / b for a, b in zip(f32, f64)])  # per epoch, larger case
    gpu = np.array(traj_gpu[case][0])
    dev = np.abs(gpu - f64[case]) / f64[case]
    print(f"trajectory {TRAJ[case]}: gpu loss {gpu[0]:.4f} -> {gpu[-1]:.4f} "
          f"(f64 {f64[case][0]:.4f} -> {f64[case][-1]:.4f})")
    for e in range(EPOCHS):
        print(f"  epoch {e + 1}: gpu dev {dev[e]:.3e}, cpu-f32 yardstick {yard[e]:.3e}, "
              f"ratio {dev[e] / yard[e]:.2f}")
    assert gpu[-1] < 0.25 * gpu[0]
    assert (dev <= FACTOR * yard).all()


def test_training_is_deterministic(traj_data, traj_gpu):
    _, _, x, y = traj_data
    dims, batch = TRAJ[0]
    losses, W, b = _gpu_traj(dims, batch, x, y)
    assert losses == traj_gpu[0][0]
    for a, r in zip(W + b, traj_gpu[0][1] + traj_gpu[0][2]):
        assert np.array_equal(a, r)


def test_epoch_losses_with_ragged_steps_and_validation_chunks():
    """13 training rows in batches of 5 (steps of 5, 5, 3 rows) and 19 validation
    rows through max_batch 8 (chunks of 8, 8, 3): both losses of two epochs
    against the float64 trainer, and the same bits from a second run."""
    from inversekinematicsann_amd import _native
    torch = _torch()
    dims, max_batch, batch, n_train, n_val = (3, 8, 4), 8, 5, 13, 19
    m = _model(dims, seed=7)
    x, y = _batch(dims, n_train, seed=8)
    xv, yv = _batch(dims, n_val, seed=9)
    rng = np.random.default_rng(1)
    perms = [rng.permutation(n_train).astype(np.int32) for _ in range(2)]

    def run():
        c = _native.Context(0)
        try:
            c.train_begin(m.weights, m.biases, m.activations, max_batch=max_batch, lr=1e-3)
            c.train_data(x, y, xv, yv)
            losses = [c.train_epoch(p, batch) for p in perms]
            W, b = c.train_get("weights")
            c.train_end()
        finally:
            c.close()
        return losses, W + b

    losses, params = run()
    tr = CpuTrainer(m.weights, m.biases, m.activations, torch.float64, lr=1e-3)
    xv64, yv64 = torch.tensor(xv, dtype=torch.float64), torch.tensor(yv, dtype=torch.float64)
    for e, p in enumerate(perms):
        tl = tr.epoch(x, y, p, batch)
        h = xv64
        for W, b, a in zip(tr.W, tr.b, tr.acts):  # the end-of-epoch weights
            h = _act(torch, a, h @ W + b)
        vl = float(((h - yv64) ** 2).sum()) / (n_val * dims[-1])
        print(f"epoch {e + 1}: loss {losses[e][0]:.9g} vs {tl:.9g} "
              f"(rel {abs(losses[e][0] - tl) / tl:.2e}), val {losses[e][1]:.9g} vs {vl:.9g} "
              f"(rel {abs(losses[e][1] - vl) / vl:.2e})")
        assert abs(losses[e][0] - tl) <= 1e-5 * abs(tl)
        assert abs(losses[e][1] - vl) <= 1e-5 * abs(vl)
    again, params2 = run()
    assert again == losses
    for a, r in zip(params2, params):
        assert np.array_equal(a, r)


# ---- 5. end to end -------------------------------------------------------------
def test_fit_end_to_end(traj_data, tmp_path):
    from inversekinematicsann_amd import _native
    from inversekinematicsann_amd.kinematics.ann import ANN
    pts, ang, _, _ = traj_data
    ann = ANN({}, [])
    hist = ann.fit(3, pts, ang, hidden=(2, 64, "tanh"), learning_rate=1e-3)
    assert len(hist["loss"]) == 3 and len(hist["val_loss"]) == 3
    assert np.isfinite(hist["val_loss"]).all() and np.isfinite(hist["loss"]).all()
    assert 0 <= hist["best_epoch"] < 3 and hist["stopped_epoch"] == 0
    assert ann.model.dims == [3, 64, 64, 4]
    assert ann.x_data_skaler.n_samples_seen == 2048 - math.ceil(0.33 * 2048)
    m = ann.model
    got = ann.predict(pts[:500])
    ref = O.ann_forward(pts[:500], m.weights, m.biases, m.activations,
                        *ann.x_data_skaler.effective(), *ann.y_data_skaler.effective())
    assert np.abs(got.astype(np.float64) - ref).max() <= 1e-5
    path = ann.save_model(str(tmp_path / "fitted"))
    back = ANN({}, [])
    back.load_model(path)
    for a, r in zip(back.model.weights + back.model.biases, m.weights + m.biases):
        assert np.array_equal(a, r)
    assert back.model.activations == m.activations
    for a, r in ((back.x_data_skaler, ann.x_data_skaler), (back.y_data_skaler, ann.y_data_skaler)):
        assert np.array_equal(a.mean, r.mean) and np.array_equal(a.scale, r.scale)
        assert np.array_equal(a.var, r.var) and a.n_samples_seen == r.n_samples_seen
    # data order, no validation rows: val_loss NaN, status OK
    c = _native.context()
    c.train_begin(m.weights, m.biases, m.activations, max_batch=32, lr=1e-3)
    try:
        _, _, x, y = traj_data
        c.train_data(x[:100], y[:100])
        loss, val = c.train_epoch(None, 32)
        assert np.isfinite(loss) and math.isnan(val)
    finally:
        c.train_end()


# ---- 6. misuse ---------------------------------------------------------------------
def test_misuse_is_badarg_and_inference_survives(ctx):
    from inversekinematicsann_amd import _native
    from inversekinematicsann_amd.kinematics.ann import glorot_model, REFERENCE_X_SCALER, \
        REFERENCE_Y_SCALER
    from inversekinematicsann_amd.robot.position_generator import random_dist
    m = glorot_model(dims=(3, 64, 64, 4), seed=1)
    sc = (REFERENCE_X_SCALER.mean, REFERENCE_X_SCALER.scale, REFERENCE_Y_SCALER.mean,
          REFERENCE_Y_SCALER.scale)
    ctx.ann_load(m.weights, m.biases, m.activations, *sc)
    x, y = _batch((3, 4), 16, seed=1)

    def badarg(fn):
        with pytest.raises(_native.NativeError) as ei:
            fn()
        assert ei.value.code == _native.IK_E_BADARG
        assert len(str(ei.value)) > len("libikhip error 16: ")
        assert ctx.lib.ik_last_error().decode()

    badarg(lambda: ctx.train_step(x, y))                       # step before begin
    badarg(lambda: ctx.train_epoch(None, 8))
    badarg(lambda: ctx.train_end())
    ctx.train_begin(m.weights, m.biases, m.activations, max_batch=8, lr=1e-3)
    badarg(lambda: ctx.train_step(x, y))                       # 16 rows > max_batch 8
    badarg(lambda: ctx.train_epoch(None, 8))                   # epoch before data
    ctx.train_data(x, y)
    badarg(lambda: ctx.train_epoch(np.arange(16)[::-1] + 1, 8))  # perm entry 16
    badarg(lambda: ctx.train_epoch(np.arange(16) - 1, 8))        # perm entry -1
    badarg(lambda: ctx.train_epoch(None, 9))                   # batch > max_batch
    assert np.isfinite(ctx.train_step(x[:8], y[:8]))
    ctx.train_end()
    pts = random_dist(1000, seed=5)
    got, _, _ = ctx.ann_solve(pts, check_limits=False)
    ref = O.ann_forward(pts, m.weights, m.biases, m.activations, *sc)
    assert np.abs(got.astype(np.float64) - ref).max() <= 1e-5
