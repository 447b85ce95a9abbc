"""The exact ANN probes (tests/ann_probes.py) on the CPU: every probe the GPU
tests rely on is exact -- its layers' spans are at most 20 bits, so any
accumulator at least as wide as fp32 gives the float64 result -- and sensitive:
a kept split product left out, an 8-deep k group or a 32-column tile zeroed
changes some output."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import ann_probes as P

ALL_CASES = sorted({c for cases in P.CASES.values() for c in cases}, key=P.case_id)
SAT = ("Bt", "Bs", "C3", "C2", "C1")  # families with a saturating layer


@pytest.mark.parametrize("case", ALL_CASES, ids=P.case_id)
def test_probe_is_exact(case):
    """Span <= 20 bits in every layer; the stored-fp32 float64 forward equals the
    plain float64 oracle bit for bit (relu / linear) or to 1e-10 (saturating:
    float64 tanh(16) is 1 - 2.5e-14, which fp32 storage rounds to 1); a float32
    numpy forward and the plane-by-plane restatements of all three modes give the
    same bits."""
    p, exp = P.expected(case)
    assert exp.shape == (P.N_PTS, 4) and np.isfinite(exp).all()
    assert np.abs(exp).max() <= 2 * np.pi  # angles the FK round trip accepts
    spans = P.span_bits(p)
    print(P.case_id(case), "span bits per layer:", [round(s, 1) for s in spans])
    assert max(spans) <= 20, spans
    with np.errstate(over="ignore"):
        plain = O.ann_forward(p.pts, p.weights, p.biases, p.acts, *P.IDENTITY, compute=np.float64)
        f32 = O.ann_forward(p.pts, p.weights, p.biases, p.acts, *P.IDENTITY, compute=np.float32)
    if case[0] in SAT:
        assert np.abs(plain.astype(np.float64) - exp).max() <= 1e-10
    else:
        assert np.array_equal(plain, exp)
    assert np.array_equal(f32, exp)
    for mode in ("fp32", "bf16x6", "fp16x3"):
        assert np.array_equal(P.forward_emulated(p, mode), exp), mode
    # not degenerate: many distinct outputs, every output column varies
    assert len(np.unique(exp)) >= (6 if case[0] in ("C3", "C2", "C1") else 40)
    assert (exp.max(axis=0) > exp.min(axis=0)).all()


@pytest.mark.parametrize("case", [c for c in ALL_CASES if c[0] in ("Bt", "Bs")], ids=P.case_id)
def test_saturating_activations_are_exact(case):
    """Family B: every hidden pre-activation is at least 16 (tanh) or 256
    (sigmoid: the fp32 exp2 overflows to inf or underflows to 0) in magnitude, the
    activations are exactly +-1 or 0 / 1, and the last hidden layer is balanced."""
    p = P.build(case)
    hs = P.layer_inputs(p)
    lo, vals = (16, (-1.0, 1.0)) if case[0] == "Bt" else (256, (0.0, 1.0))
    for l, h in enumerate(hs[:-1]):
        z = h.astype(np.float64) @ p.weights[l].astype(np.float64) + p.biases[l]
        assert np.abs(z).min() >= lo, (l, np.abs(z).min())
        if case[0] == "Bs":  # what the kernel computes in fp32: 1 / (1 + exp2(-log2(e) z))
            with np.errstate(over="ignore"):
                e = np.exp2((np.float32(-1.4426950408889634) * z.astype(np.float32)))
            assert np.all((e == 0) | np.isinf(e))
    for h in hs[1:]:
        assert np.isin(h, vals).all()
    assert 0.3 <= (hs[-1] == vals[1]).mean() <= 0.7


@pytest.mark.parametrize("case", [c for c in ALL_CASES if c[0] == "C3"], ids=P.case_id)
def test_three_part_weights_fill_every_plane(case):
    """Family C: every plane of every nonzero weight of the probed layer is
    nonzero, in the bf16 split (1, 2^-9, 2^-17 times s) and in the fp16 split of
    the pre-scaled weight (8208 and 0.0625 for s = 1)."""
    W = P.build(case).weights[1]
    nz = W != 0
    assert nz.sum() == 2 * W.shape[1]
    for plane in P.bf16_split3(W):
        assert (plane[nz] != 0).all()
    hi, mid, lo = P.bf16_split3(W)
    assert np.array_equal(hi.astype(np.float64) + mid + lo, W.astype(np.float64))
    assert set(np.abs(hi[nz])) == {1.0, 0.5}
    s = P.h_scale_exp(W)
    assert s == 13
    h_hi, h_lo = P.f16_split2(np.ldexp(W, s))
    assert (h_hi[nz] != 0).all() and (h_lo[nz] != 0).all()
    assert set(np.abs(h_hi[nz])) == {8208.0, 4104.0} and set(np.abs(h_lo[nz])) == {0.0625, 0.03125}
    assert np.array_equal(h_hi.astype(np.float64) + h_lo, np.ldexp(W.astype(np.float64), s))


@pytest.mark.parametrize("case", [c for c in ALL_CASES if c[0] == "C2"], ids=P.case_id)
def test_two_part_operands(case):
    """Family C, two-part times two-part: the probed layer's weights and its
    nonzero input activations are +-(1 + 2^-8): bf16 hi 1, mid 2^-8, no lo."""
    p = P.build(case)
    W, x = p.weights[2], P.layer_inputs(p)[2]
    for v in (W[W != 0], x[x != 0]):
        hi, mid, lo = P.bf16_split3(v)
        assert len(v) and set(np.abs(hi)) == {1.0} and set(np.abs(mid)) == {2.0 ** -8}
        assert not lo.any()
    assert (x != 0).any(axis=0).mean() >= 0.5  # most k carry a value for some point


def _split_cases(mode):
    """The cases with at least one layer that runs `mode`'s split GEMM."""
    out = []
    for path, cases in P.CASES.items():
        for fam, dims in cases:
            acts = P.build((fam, dims), n=8).acts
            if any(P.layer_kind(dims, acts, l, mode) == mode for l in range(len(dims) - 1)):
                out.append((fam, dims))
    return out


@pytest.mark.parametrize("mode,drop", [("bf16x6", i) for i in range(6)] +
                         [("fp16x3", i) for i in range(3)])
def test_dropped_product_is_seen(mode, drop):
    """Leaving one kept product out of the split GEMMs changes some probe's
    output -- except fp16x3's X.lo * W.hi, which no exact probe can reach: an
    activation with a nonzero fp16 lo part after tanh or sigmoid (the only inputs
    of an fp16x3 layer) is not exactly known.  That product stays with the
    tolerance tests and the invariance tests of tests/test_gpu_ann_probes.py."""
    seen = []
    for case in _split_cases(mode):
        if len(case[1]) > 8 or max(case[1]) > 1100:
            continue  # the small shapes suffice
        p, exp = P.expected(case)
        if not np.array_equal(P.forward_emulated(p, mode, drop=drop), exp):
            seen.append(P.case_id(case))
    kept = (P.BF16_KEPT if mode == "bf16x6" else P.F16_KEPT)[drop]
    print(mode, "without W plane %d x X plane %d: seen by" % kept, seen)
    if mode == "fp16x3" and kept == (0, 1):
        assert not seen
    else:
        assert seen


def test_dropped_product_families():
    """Which family reaches which bf16x6 product: the dyadic models W.hi times
    X.hi and X.mid, the three-part activations X.lo, the three-part weights W.mid
    and W.lo times X.hi, the two-part probe mid * mid."""
    def seen(case, drop):
        p, exp = P.expected(case)
        return not np.array_equal(P.forward_emulated(p, "bf16x6", drop=drop), exp)
    a, c3, c2 = ("A", (3, 100, 37, 250, 4)), ("C3", (3, 250, 100, 4)), ("C2", (3, 128, 96, 64, 4))
    idx = {k: i for i, k in enumerate(P.BF16_KEPT)}
    assert seen(a, idx[(0, 0)]) and seen(a, idx[(0, 1)])
    assert seen(("C1", (3, 128, 96, 64, 4)), idx[(0, 2)])
    assert seen(c3, idx[(1, 0)]) and seen(c3, idx[(2, 0)])
    assert seen(c2, idx[(1, 1)])


@pytest.mark.parametrize("case", [c for c in ALL_CASES if c[0] in ("A", "Bt", "Bs")], ids=P.case_id)
def test_every_k_group_and_column_tile_is_seen(case):
    """Zeroing any single 8-deep k group or any single 32-column tile of any
    hidden layer's weights changes some output (96 points)."""
    p = P.build(case, n=96)
    exp = P.forward_f64_stored_f32(p.weights, p.biases, p.acts, p.pts)
    hs = P.layer_inputs(p)
    missed = []
    for l in range(1, len(p.weights) - 1):
        W, x = p.weights[l].astype(np.float64), hs[l].astype(np.float64)
        K, N = W.shape
        z = x @ W + p.biases[l]  # exact in float64, and so is taking a block's terms out again
        blocks = [("k", slice(g, g + 8), slice(None)) for g in range(0, K, 8)] + \
                 [("n", slice(None), slice(t, t + 32)) for t in range(0, N, 32)]
        for what, ks, ns in blocks:
            z2 = z.copy()
            z2[:, ns] -= x[:, ks] @ W[ks, ns]
            out = P.forward_f64_stored_f32(p.weights, p.biases, p.acts, None, start=l + 1,
                                           h=P._activate(p.acts[l], z2).astype(np.float32))
            if np.array_equal(out, exp):
                missed.append((l, what, ks.start if what == "k" else ns.start))
    assert not missed, missed[:20]
