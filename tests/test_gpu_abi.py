"""C-ABI argument checking on a live context (include/ikhip.h): every entry
point refuses bad arguments with IK_E_BADARG / IK_E_NOMODEL and a message in
ik_last_error(), leaves the context usable, and never launches a kernel on a
rejected call.  The Python wrappers surface these as NativeError."""
import ctypes

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from inversekinematicsann_amd import _native
    c = _native.Context(0)
    yield c
    c.close()


def _rc_msg(ctx, rc):
    return rc, ctx.lib.ik_last_error().decode()


def test_bad_arguments_are_refused(ctx):
    from inversekinematicsann_amd import _native as N
    L, h = ctx.lib, ctx.handle
    st = N.IkStats()
    pts = np.zeros((4, 3))
    ang = np.zeros((4, 4))
    # negative sizes / null pointers
    rc, msg = _rc_msg(ctx, L.ik_fabrik_solve(h, pts.ctypes.data, -1, 1e-3, 100, ang.ctypes.data,
                                             None, None, 0, ctypes.byref(st)))
    assert rc == N.IK_E_BADARG and "ik_fabrik_solve" in msg
    rc, msg = _rc_msg(ctx, L.ik_fabrik_solve(h, None, 4, 1e-3, 100, ang.ctypes.data, None, None,
                                             0, ctypes.byref(st)))
    assert rc == N.IK_E_BADARG
    rc, msg = _rc_msg(ctx, L.ik_fk(h, ang.ctypes.data, 4, None, None, 0, ctypes.byref(st)))
    assert rc == N.IK_E_BADARG and "ik_fk" in msg
    rc, msg = _rc_msg(ctx, L.ik_check_limits(h, None, 3, 0, ctypes.byref(st)))
    assert rc == N.IK_E_BADARG
    # async without device pointers
    rc, msg = _rc_msg(ctx, L.ik_fabrik_solve(h, pts.ctypes.data, 4, 1e-3, 100, ang.ctypes.data,
                                             None, None, N.IK_F_ASYNC, ctypes.byref(st)))
    assert rc == N.IK_E_BADARG and "IK_F_ASYNC" in msg
    # device outputs the kernels store 16 bytes at a time must be 16-byte aligned
    import torch
    dp = torch.zeros((4, 3), dtype=torch.float64, device="cuda")
    da = torch.zeros(17, dtype=torch.float64, device="cuda")
    rc, msg = _rc_msg(ctx, L.ik_fabrik_solve(h, dp.data_ptr(), 4, 1e-3, 100,
                                             da.data_ptr() + 8, None, None, N.IK_F_DEVICE,
                                             ctypes.byref(st)))
    assert rc == N.IK_E_BADARG and "aligned" in msg
    # generic chains: at least one joint
    rc, msg = _rc_msg(ctx, L.ik_fabrik_calc(h, 0, pts.ctypes.data, pts.ctypes.data, 1,
                                            pts.ctypes.data, 4, 1e-3, 100, ang.ctypes.data,
                                            None, 0, ctypes.byref(st)))
    assert rc == N.IK_E_BADARG and "nj" in msg
    # unknown ANN mode
    rc, msg = _rc_msg(ctx, L.ik_ann_set_mode(h, 7))
    assert rc == N.IK_E_BADARG and "mode" in msg
    # the context still works
    p = np.array([[1.0, 2.1, 3.0]])
    a, it, _, s = ctx.fabrik_solve(p)
    ra, rit, _, _ = O.fabrik_ikine(p)
    assert np.array_equal(it, rit) and np.abs(a - ra).max() <= 1e-9


def test_ann_without_model_and_bad_models():
    from inversekinematicsann_amd import _native as N
    from inversekinematicsann_amd.kinematics.ann import REFERENCE_X_SCALER as XS, \
        REFERENCE_Y_SCALER as YS
    c = N.Context(0)
    try:
        with pytest.raises(N.NativeError) as ei:
            c.ann_solve(np.zeros((3, 3)))
        assert ei.value.code == N.IK_E_NOMODEL
        rng = np.random.default_rng(0)

        def dense(i, o):
            return rng.standard_normal((i, o)).astype(np.float32), np.zeros(o, np.float32)

        # wider than the layered path takes (16384), wrong input / output widths
        for dims in ((3, 16385, 4), (4, 16, 4), (3, 16, 5)):
            ws, bs = zip(*[dense(dims[k], dims[k + 1]) for k in range(len(dims) - 1)])
            with pytest.raises(N.NativeError) as ei:
                c.ann_load(list(ws), list(bs), ["tanh"] * (len(dims) - 2) + ["linear"], XS.mean,
                           XS.scale, YS.mean, YS.scale)
            assert ei.value.code == N.IK_E_BADARG
        # after the refusals a valid model loads and solves
        ws, bs = zip(*[dense(3, 32), dense(32, 4)])
        c.ann_load(list(ws), list(bs), ["tanh", "linear"], XS.mean, XS.scale, YS.mean, YS.scale)
        pts = np.array([[1.0, 0.5, 2.0], [0.3, -0.2, 1.0]])
        ang, _, _ = c.ann_solve(pts)
        ref = O.ann_forward(pts, list(ws), list(bs), ["tanh", "linear"], XS.mean, XS.scale,
                            YS.mean, YS.scale)
        assert np.abs(ang.astype(np.float64) - ref).max() <= 1e-5
    finally:
        c.close()


def test_bad_device_index():
    from inversekinematicsann_amd import _native as N
    L = N.load_library()
    h = ctypes.c_void_p()
    rc = L.ik_ctx_create(4096, ctypes.byref(h))
    assert rc == N.IK_E_BADARG and not h.value
    assert b"out of range" in L.ik_last_error()


def test_ann_effective_mode_reports_the_arithmetic_run():
    """ik_ann_effective_mode: the set mode when the model has layers
    that take it, fp32 for a fused model wider than 512 (with a RuntimeWarning from
    the Python wrapper), bf16x6 for fp16x3 on the layered path; -IK_E_NOMODEL
    before a model is loaded."""
    import warnings
    from inversekinematicsann_amd import _native as N
    from inversekinematicsann_amd.kinematics.ann import (REFERENCE_X_SCALER as XS,
                                                         REFERENCE_Y_SCALER as YS, glorot_model)
    c = N.Context(0)
    try:
        assert c.lib.ik_ann_effective_mode(c.handle) == -N.IK_E_NOMODEL

        def load(dims):
            m = glorot_model(dims, seed=1)
            c.ann_load(m.weights, m.biases, m.activations, XS.mean, XS.scale, YS.mean, YS.scale)

        load((3, 64, 64, 4))
        for mode in ("fp32", "bf16x6", "fp16x3"):
            c.ann_set_mode(mode)
            assert c.ann_effective_mode() == mode
        c.ann_set_mode("bf16x6")
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            load((3, 600, 600, 4))          # fused, wider than 512: fp32 build
        assert c.ann_effective_mode() == "fp32"
        assert any("ik_ann_effective_mode" in str(x.message) for x in w)
        c.ann_set_mode("fp16x3")
        load((3,) + (64,) * 30 + (4,))      # past the fused kernel's 24 layers: layered
        assert c.ann_effective_mode() == "bf16x6"
        pts = np.array([[1.0, 0.5, 2.0], [0.3, -0.2, 1.0]])
        ang, _ = c.ann_solve(pts)[:2]
        assert np.isfinite(ang).all()
    finally:
        c.close()


def test_kernel_timing_per_call_and_accumulated(ctx):
    """ik_ctx_set_timing: on = 1 keeps the last call's kernels, on = 2 accumulates
    the calls' kernels in launch order (what bench.timed uses to time back-to-back
    steps with no host sync between them); every duration is positive and the
    accumulated run repeats the one-call sequence."""
    from inversekinematicsann_amd.robot.position_generator import random_dist
    pts = random_dist(50_000, seed=5)
    ctx.set_timing(True)
    ctx.fabrik_solve(pts, 1e-3, 100)
    ctx.fabrik_solve(pts, 1e-3, 100)
    one = ctx.kernel_times()
    ctx.set_timing(2)
    for _ in range(3):
        ctx.fabrik_solve(pts, 1e-3, 100)
    acc = ctx.kernel_times()
    ctx.set_timing(False)
    assert ctx.kernel_times() == []
    names = [k for k, _ in one]
    assert "fabrik_iter_kernel" in names
    assert [k for k, _ in acc] == names * 3
    assert all(ms > 0.0 for _, ms in one + acc)


# ---- host pointers == device pointers ------------------------------------------
# Every solve takes host arrays (staged through the context's scratch) or device
# arrays (IK_F_DEVICE).  The two must return the same bytes and the same stats,
# whichever optional outputs the caller asks for.

_F64, _F32, _I32 = np.float64, np.float32, np.int32
_CHAIN_DH = np.array([[0.0, 0.0, 0.0], [0.5, 0.0, 0.3], [0.0, 1.5, 1.0],
                      [np.pi / 2, 0.0, 0.0]])           # 4 x nj, nj = 3
_CHAIN_LINKS = np.array([1.0, 0.75, 0.5])
_STAT_FIELDS = ("first_oob", "first_err", "first_err_code", "max_iters", "sum_iters",
                "n_capped", "max_fk_err")                # (sum_fk_err: atomic order not fixed)


def _points(n):
    from inversekinematicsann_amd.robot.position_generator import random_dist
    pts = random_dist(n, seed=11)
    if n > 5:
        pts[5] = (-1.0, 0.0, 0.0)                        # outside the workspace: first_oob
    return pts


def _parity_cases():
    """name -> (inputs(n), outputs(n), optional output names, call(L, h, p, n, flags, st));
    inputs: name -> (array, always_host); outputs: name -> (shape, dtype)."""
    rng = np.random.default_rng(3)

    def ang4(n):
        return rng.uniform(-1.0, 1.0, (n, 4))

    def calc_in(n, shared):
        init = np.zeros((3, 3))
        init[:, 2] = np.cumsum(_CHAIN_LINKS)
        goals = rng.uniform(-1.0, 1.0, (n, 3)) + (0.0, 0.0, 1.0)
        return {"dists": (_CHAIN_LINKS, True), "goals": (goals, False),
                "init": (init if shared else np.tile(init, (n, 1, 1)), False)}

    def calc(shared):
        return (lambda n: calc_in(n, shared),
                lambda n: {"joints": ((n, 3, 3), _F64), "iters": ((n,), _I32)}, ("iters",),
                lambda L, h, p, n, f, st: L.ik_fabrik_calc(
                    h, 3, p("dists"), p("init"), int(shared), p("goals"), n, 1e-3, 50,
                    p("joints"), p("iters"), f, st))

    pts_in = lambda n: {"pts": (_points(n), False)}      # noqa: E731
    refined_out = lambda n: {"ang": ((n, 4), _F64), "iters": ((n,), _I32),   # noqa: E731
                             "fk_err": ((n,), _F64)}
    return {
        "check_limits": (pts_in, lambda n: {}, (),
                         lambda L, h, p, n, f, st: L.ik_check_limits(h, p("pts"), n, f, st)),
        "fk": (lambda n: {"ang": (ang4(n), False)},
               lambda n: {"xyz": ((n, 3), _F64), "mats": ((n, 4, 4, 4), _F64)}, ("mats",),
               lambda L, h, p, n, f, st: L.ik_fk(h, p("ang"), n, p("xyz"), p("mats"), f, st)),
        "fk_chain": (lambda n: {"dh": (_CHAIN_DH, True), "ang": (ang4(n)[:, :3].copy(), False)},
                     lambda n: {"xyz": ((n, 3), _F64), "mats": ((n, 3, 4, 4), _F64)}, ("mats",),
                     lambda L, h, p, n, f, st: L.ik_fk_chain(h, 3, p("dh"), p("ang"), n, p("xyz"),
                                                             p("mats"), f, st)),
        "fabrik_solve_fk": (pts_in,
                            lambda n: {"ang": ((n, 4), _F64), "iters": ((n,), _I32),
                                       "joints": ((n, 4, 3), _F64), "fk_err": ((n,), _F64)},
                            ("iters", "joints", "fk_err"),
                            lambda L, h, p, n, f, st: L.ik_fabrik_solve_fk(
                                h, p("pts"), n, 1e-3, 100, p("ang"), p("iters"), p("joints"),
                                p("fk_err"), f, st)),
        "fabrik_calc": calc(False),
        "fabrik_calc_shared": calc(True),
        "ann_solve": (pts_in, lambda n: {"ang": ((n, 4), _F32), "fk_err": ((n,), _F64)},
                      ("fk_err",),
                      lambda L, h, p, n, f, st: L.ik_ann_solve(h, p("pts"), n, p("ang"),
                                                               p("fk_err"), f, st)),
        "refine": (lambda n: {"pts": (_points(n), False), "seed": (ang4(n), False)},
                   refined_out, ("iters", "fk_err"),
                   lambda L, h, p, n, f, st: L.ik_refine(h, p("pts"), p("seed"), n, 1e-6, 20, 1e-3,
                                                         p("ang"), p("iters"), p("fk_err"), f, st)),
        "ann_solve_refined": (pts_in,
                              lambda n: {**refined_out(n), "seed_fk_err": ((n,), _F64)},
                              ("iters", "fk_err", "seed_fk_err"),
                              lambda L, h, p, n, f, st: L.ik_ann_solve_refined(
                                  h, p("pts"), n, 1e-6, 20, 1e-3, p("ang"), p("iters"),
                                  p("fk_err"), p("seed_fk_err"), f, st)),
    }


_PARITY = _parity_cases()


def _parity_params():
    """Every optional output once present and once absent: all, none, and (where a
    call has several) each one alone."""
    out = []
    for name, case in _PARITY.items():
        opt = case[2]
        masks = [opt, ()] + ([(o,) for o in opt] if len(opt) > 1 else [])
        for want in masks if opt else [()]:
            for n in (0, 1, 257):
                out.append(pytest.param(name, n, want, id=f"{name}-{n}-{'+'.join(want) or 'none'}"))
    return out


def _run(ctx, call, ins, outs, n, device):
    """One call with host or device arrays: (outputs as numpy arrays, stats)."""
    import torch
    from inversekinematicsann_amd import _native as N
    st = N.IkStats()
    hold = {}
    for k, (a, always_host) in ins.items():
        a = np.ascontiguousarray(a)
        hold[k] = torch.from_numpy(a).cuda() if device and not always_host else a
    for k, (shape, dt) in outs.items():
        a = np.full(shape, -7, dt)                       # the same fill on both paths
        hold[k] = torch.from_numpy(a).cuda() if device else a
    torch.cuda.synchronize()
    rc = call(ctx.lib, ctx.handle, lambda k: N._ptr(hold.get(k)), n,
              N.IK_F_DEVICE if device else 0, ctypes.byref(st))
    assert rc == N.IK_OK, ctx.lib.ik_last_error().decode()
    return {k: (hold[k].cpu().numpy() if device else hold[k]) for k in outs}, st


def _same_bytes(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(
        a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8))


@pytest.fixture(scope="module")
def model_ctx():
    from inversekinematicsann_amd import _native
    from inversekinematicsann_amd.kinematics.ann import (REFERENCE_X_SCALER as XS,
                                                         REFERENCE_Y_SCALER as YS, glorot_model)
    c = _native.Context(0)
    m = glorot_model((3, 32, 4), seed=1)
    c.ann_load(m.weights, m.biases, m.activations, XS.mean, XS.scale, YS.mean, YS.scale)
    yield c
    c.close()


@pytest.mark.parametrize("name,n,want", _parity_params())
def test_host_pointers_equal_device_pointers(model_ctx, name, n, want):
    """The host-pointer call and the IK_F_DEVICE call on the same inputs return
    bit-identical arrays and equal stats, for n = 0, 1 and 257 (one full
    256-thread block and a row) and with each optional output present and absent."""
    make_in, make_out, optional, call = _PARITY[name]
    ins = make_in(n)
    outs = {k: v for k, v in make_out(n).items() if k not in optional or k in want}
    host, hst = _run(model_ctx, call, ins, outs, n, device=False)
    dev, dst = _run(model_ctx, call, ins, outs, n, device=True)
    for k in outs:
        assert _same_bytes(host[k], dev[k]), k
        if n:
            assert not (host[k] == -7).all(), k          # the call wrote it
    for f in _STAT_FIELDS:
        assert getattr(hst, f) == getattr(dst, f), (f, hst.as_dict(), dst.as_dict())
    if n == 257 and "pts" in ins and name != "refine":
        assert hst.first_oob == 5


def test_host_staging_survives_a_growing_scratch():
    """A fresh context's first host-pointer FABRIK call sizes the scratch for one
    row; the next one's staging exceeds that allocation, so the scratch is
    reallocated.  Both equal the device path (pointers into the old allocation
    would not)."""
    from inversekinematicsann_amd import _native
    make_in, make_out, _, call = _PARITY["fabrik_solve_fk"]
    c = _native.Context(0)
    try:
        got = [_run(c, call, make_in(n), make_out(n), n, device=False) for n in (1, 40_000)]
        for (host, hst), n in zip(got, (1, 40_000)):
            dev, dst = _run(c, call, make_in(n), make_out(n), n, device=True)
            for k in host:
                assert _same_bytes(host[k], dev[k]), (n, k)
            for f in _STAT_FIELDS:
                assert getattr(hst, f) == getattr(dst, f), (n, f)
    finally:
        c.close()
