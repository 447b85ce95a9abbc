"""The ANN kernels against expected outputs that are known exactly, and against
themselves under transformations that must not change a bit -- no tolerance for
a wrong index, a dropped plane or a row-dependent layout to hide in.

Probes (tests/ann_probes.py, proven exact and sensitive on the CPU by
tests/test_ann_probes_cpu.py): np.array_equal against a float64 forward on the
fused, wide and layered paths in every arithmetic mode and at both tile sizes.
Invariance (Glorot models, no reference needed): the same bits for a point
wherever it sits in the batch and whatever the batch size, beside non-finite
rows, and under power-of-two rescaling of a layer."""
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

from oracle import oracle as O
from tests import ann_probes as P
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

NS_TOL = 1e-5
ALL_MODES = ("fp32", "bf16x6", "fp16x3")


@pytest.fixture(scope="module")
def ctx1():
    from inversekinematicsann_amd import _native
    c = _native.Context(0)
    yield c
    c.close()


def _set_mode(ctx, mode):
    with warnings.catch_warnings():  # "mode not available for the loaded model": asserted here
        warnings.simplefilter("ignore", RuntimeWarning)
        ctx.ann_set_mode(mode)


def _load(ctx, weights, biases, acts, scalers):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        ctx.ann_load(weights, biases, acts, *scalers)


def _fk_err(ang, pts):
    return np.linalg.norm(O.fk_closed_form(ang.astype(np.float64)) - pts, axis=1)


def _differs(got, exp):
    rows = np.flatnonzero((got != exp).any(axis=1))
    return f"{len(rows)} rows differ, first {rows[:6].tolist()}: got {got[rows[:2]].tolist()} " \
           f"expected {exp[rows[:2]].tolist()}"


# ---------------------------------------------------------- exact probes ----
@pytest.mark.parametrize("path,case", [(p, c) for p in P.CASES for c in P.CASES[p]],
                         ids=lambda v: v if isinstance(v, str) else P.case_id(v))
def test_probe_bits(ctx1, path, case):
    """Every mode of the path gives the float64 forward's bits, and fk_err the
    float64 FK round trip of those angles."""
    p, exp = P.expected(case)
    fk_ref = _fk_err(exp, p.pts)
    _load(ctx1, p.weights, p.biases, p.acts, P.IDENTITY)
    try:
        for mode in P.MODES[path]:
            _set_mode(ctx1, mode)
            if mode != "fp32" and path in P.EFFECTIVE:
                assert ctx1.ann_effective_mode() == P.EFFECTIVE[path][mode]
            ang, err, _ = ctx1.ann_solve(p.pts, check_limits=False, want_fk_err=True)
            assert np.array_equal(ang, exp), f"{mode}: " + _differs(ang, exp)
            assert np.abs(err - fk_ref).max() <= 1e-9, mode
    finally:
        ctx1.ann_set_mode("fp32")


_OTHER_TILE = """
import sys
import warnings
import numpy as np
from inversekinematicsann_amd import _native
from tests import ann_probes as P
mode, out = sys.argv[1], sys.argv[2]
warnings.simplefilter("ignore", RuntimeWarning)
c = _native.Context(0)
res = {}
for i, case in enumerate(P.CASES["fused"]):
    p = P.build(case)
    c.ann_load(p.weights, p.biases, p.acts, *P.IDENTITY)
    c.ann_set_mode(mode)
    a, e, _ = c.ann_solve(p.pts, check_limits=False, want_fk_err=True)
    c.ann_set_mode("fp32")
    res["a%d" % i], res["e%d" % i] = a, e
np.savez(out, **res)
"""


@pytest.mark.parametrize("mode", ALL_MODES)
def test_probe_bits_other_tile(tmp_path, mode):
    """The fused probes at the other tile size (IKHIP_ANN_MR, read once per
    process: a fresh child), 64-point tiles for fp32 and 32-point ones for the
    split modes."""
    out = tmp_path / "other.npz"
    r = subprocess.run([sys.executable, "-c", _OTHER_TILE, mode, str(out)], cwd=ROOT,
                       capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, IKHIP_ANN_MR="2" if mode == "fp32" else "1"))
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.load(out)
    for i, case in enumerate(P.CASES["fused"]):
        p, exp = P.expected(case)
        assert np.array_equal(got[f"a{i}"], exp), f"{P.case_id(case)}: " + _differs(got[f"a{i}"], exp)
        assert np.abs(got[f"e{i}"] - _fk_err(exp, p.pts)).max() <= 1e-9, P.case_id(case)


# ------------------------------------------- Glorot models, one per path ----
GLOROT = {"fused": (P.DEEP, "tanh"), "wide": ((3, 768, 500, 4), "tanh"),
          "layered": ((3, 1100, 200, 37, 4), "relu")}
PATH_MODES = [(p, m) for p in GLOROT for m in ALL_MODES]
_glorot = {}


def _glorot_case(path):
    """(model, scalers, 611 random_dist points) of a path, as test_gpu_parity's _ann_case."""
    if path not in _glorot:
        from inversekinematicsann_amd.kinematics.ann import glorot_model, REFERENCE_X_SCALER as XS, \
            REFERENCE_Y_SCALER as YS
        from inversekinematicsann_amd.robot.position_generator import random_dist
        dims, act = GLOROT[path]
        m = glorot_model(dims=dims, seed=len(dims), hidden_act=act)
        rng = np.random.default_rng(len(dims))
        for b in m.biases:
            b[:] = rng.normal(0, 0.1, b.shape).astype(np.float32)
        _glorot[path] = (m, (XS.mean, XS.scale, YS.mean, YS.scale), random_dist(P.N_PTS, seed=17))
    return _glorot[path]


@pytest.mark.parametrize("path,mode", PATH_MODES)
def test_position_and_batch_size_invariance(ctx1, monkeypatch, path, mode):
    """A point's angles and fk_err do not depend on the batch size or on its row:
    prefixes of every size around the 32 / 64 / 128 / 256-row tiles and windows
    that move each point in and out of the swizzled rows 4..11 of a 16-row block
    and between the halves of a 32-row group give the bits of the 611-point solve;
    the batch stats of 1, 31 and 33 points (a half-empty wave) match their rows."""
    m, sc, pts = _glorot_case(path)
    _load(ctx1, m.weights, m.biases, m.activations, sc)
    try:
        _set_mode(ctx1, mode)
        full, ferr, _ = ctx1.ann_solve(pts, check_limits=False, want_fk_err=True)
        assert np.isfinite(full).all() and np.isfinite(ferr).all()
        for n in (0, 1, 31, 32, 33, 63, 64, 65, 127, 129, 257):
            ang, err, st = ctx1.ann_solve(pts[:n], check_limits=False, want_fk_err=True)
            assert ang.shape == (n, 4) and err.shape == (n,)
            assert np.array_equal(ang, full[:n]), f"prefix {n}: " + _differs(ang, full[:n])
            assert np.array_equal(err, ferr[:n]), f"prefix {n}"
            if n in (1, 31, 33):
                assert st.max_fk_err == err.max(), n
                assert abs(st.sum_fk_err - err.sum()) <= 1e-9 * err.sum(), n
        for s in (1, 5, 12, 37):
            ang, err, _ = ctx1.ann_solve(pts[s:s + 70], check_limits=False, want_fk_err=True)
            assert np.array_equal(ang, full[s:s + 70]), f"window {s}: " + _differs(ang, full[s:s + 70])
            assert np.array_equal(err, ferr[s:s + 70]), f"window {s}"
        if path == "layered":
            monkeypatch.setenv("IKHIP_ANN_ACT_MB", "1")
            ang, err, _ = ctx1.ann_solve(pts[5:75], check_limits=False, want_fk_err=True)
            assert np.array_equal(ang, full[5:75]) and np.array_equal(err, ferr[5:75])
    finally:
        ctx1.ann_set_mode("fp32")


@pytest.mark.parametrize("path,mode", PATH_MODES)
def test_non_finite_rows_stay_alone(ctx1, path, mode):
    """A NaN row and two rows of +-1e300 (rows 3, 9 and 40 of the third 64-point
    tile) leave every other row's bits alone; their own outputs are NaN where the
    float64 oracle's are and within 1e-5 of it elsewhere; max_fk_err is the
    maximum over the finite rows; first_oob is the oracle's."""
    m, sc, pts = _glorot_case(path)
    rows = [128 + 3, 128 + 9, 128 + 40]
    bad = pts.copy()
    bad[rows[0]] = (np.nan, 1.0, 1.0)
    bad[rows[1]] = (1e300, 1.0, 1.0)
    bad[rows[2]] = (1.0, -1e300, 1.0)
    with np.errstate(all="ignore"):
        ref = O.ann_forward(bad[rows], m.weights, m.biases, m.activations, *sc, compute=np.float64)
    _load(ctx1, m.weights, m.biases, m.activations, sc)
    try:
        _set_mode(ctx1, mode)
        clean, cerr, _ = ctx1.ann_solve(pts, check_limits=False, want_fk_err=True)
        ang, err, st = ctx1.ann_solve(bad, check_limits=True, want_fk_err=True)
    finally:
        ctx1.ann_set_mode("fp32")
    others = np.setdiff1d(np.arange(len(pts)), rows)
    assert np.array_equal(ang[others], clean[others]), _differs(ang[others], clean[others])
    assert np.array_equal(err[others], cerr[others])
    print(f"{path} {mode}: rows {ang[rows].tolist()} oracle {ref.tolist()} fk_err {err[rows].tolist()}")
    assert np.array_equal(np.isnan(ang[rows]), np.isnan(ref)), (ang[rows], ref)
    fin = ~np.isnan(ref)
    assert np.abs(ang[rows][fin].astype(np.float64) - ref[fin]).max(initial=0.0) <= NS_TOL
    assert st.max_fk_err == err[np.isfinite(err)].max()
    assert st.first_oob == O.check_limits(bad) == rows[1]


# ------------------------------------------------ power-of-two rescaling ----
F_DIMS, F_ACTS = (3, 200, 160, 96, 4), ["tanh", "relu", "linear", "linear"]


def _rescaled(k=0, zero_hidden=False, cut_inputs=False):
    """Glorot (3, 200 tanh, 160 relu, 96 linear, 4) with the relu layer's W, b
    times 2^k and the next layer's W times 2^-k (exact in fp32, and
    relu(2^k z) = 2^k relu(z)).  zero_hidden: the relu layer's W all zero;
    cut_inputs: instead the layer before it outputs 0 (W, b zero: tanh(0) = 0)."""
    from inversekinematicsann_amd.kinematics.ann import glorot_model
    m = glorot_model(dims=F_DIMS, seed=23)
    rng = np.random.default_rng(23)
    Ws = [W.copy() for W in m.weights]
    bs = [rng.normal(0, 0.1, b.shape).astype(np.float32) for b in m.biases]
    Ws[1], bs[1], Ws[2] = np.ldexp(Ws[1], k), np.ldexp(bs[1], k), np.ldexp(Ws[2], -k)
    assert all(np.isfinite(a).all() and (np.abs(a[a != 0]) > 1e-35).all() for a in Ws + bs)
    if zero_hidden:
        Ws[1][:] = 0
    if cut_inputs:
        Ws[0][:] = 0
        bs[0][:] = 0
    return Ws, bs


def _solve_all_modes(ctx, Ws, bs, pts, sc):
    _load(ctx, Ws, bs, F_ACTS, sc)
    out = {}
    try:
        for mode in ALL_MODES:
            _set_mode(ctx, mode)
            out[mode] = (ctx.ann_solve(pts, check_limits=False)[0], ctx.ann_effective_mode())
    finally:
        ctx.ann_set_mode("fp32")
    return out


def test_power_of_two_rescaling(ctx1):
    """Scaling a relu layer by 2^k and the next by 2^-k changes no bit in any
    mode, k = -40 and +40: in fp16x3 the layer (its input is a tanh layer's) takes
    the split GEMM, its weight pre-scale exponent moves by -k and the epilogue's
    `pre` by 2^k; in bf16x6 all three planes of both layers move with the exponent."""
    _, sc, pts = _glorot_case("fused")
    base = _solve_all_modes(ctx1, *_rescaled(0), pts, sc)
    assert base["fp16x3"][1] == "fp16x3" and base["bf16x6"][1] == "bf16x6"
    for k in (-40, 40):
        got = _solve_all_modes(ctx1, *_rescaled(k), pts, sc)
        for mode in ALL_MODES:
            assert got[mode][1] == base[mode][1]
            assert np.array_equal(got[mode][0], base[mode][0]), \
                f"k {k} {mode}: " + _differs(got[mode][0], base[mode][0])


def test_all_zero_hidden_weights(ctx1):
    """An all-zero hidden weight matrix (pre-scale exponent 0, zero planes) gives
    the bits of the model whose inputs to that layer are cut, in all modes."""
    _, sc, pts = _glorot_case("fused")
    zero = _solve_all_modes(ctx1, *_rescaled(0, zero_hidden=True), pts, sc)
    cut = _solve_all_modes(ctx1, *_rescaled(0, cut_inputs=True), pts, sc)
    for mode in ALL_MODES:
        assert np.isfinite(zero[mode][0]).all()
        assert np.array_equal(zero[mode][0], cut[mode][0]), mode
        assert len(np.unique(zero[mode][0], axis=0)) == 1  # no input reaches the output


def test_weights_past_the_fp16_prescale_range(ctx1):
    """k = +90: the relu layer's largest |w| is ~2^87, past what the fp16x3
    pre-scale exponent (+-60) can bring to 2^13 -- clamped, the planes held inf.
    The layer has no fp16x3 operand and runs fp32: the only layer of this model
    that could take the split GEMM, so fp16x3 mode gives the fp32 mode's bits,
    finite and within the split modes' bound of a float64 forward."""
    _, sc, pts = _glorot_case("fused")
    Ws, bs = _rescaled(90)
    got = _solve_all_modes(ctx1, Ws, bs, pts, sc)
    ref64 = O.ann_forward(pts, Ws, bs, F_ACTS, *sc, compute=np.float64)
    ang_f, ang_h = got["fp32"][0], got["fp16x3"][0]
    assert got["fp16x3"][1] == "fp32"
    assert np.isfinite(ang_h).all()
    assert np.array_equal(ang_h, ang_f), _differs(ang_h, ang_f)
    d_f = np.abs(ang_f.astype(np.float64) - ref64).max()
    d_h = np.abs(ang_h.astype(np.float64) - ref64).max()
    assert d_h <= NS_TOL and d_h <= 4 * d_f + 2e-7, (d_h, d_f)
    # and the rescaling itself changes no bit in fp32 mode
    base = _solve_all_modes(ctx1, *_rescaled(0), pts, sc)
    assert np.array_equal(ang_f, base["fp32"][0])
