"""Probe models for the ANN kernels whose output is known exactly, and numpy
restatements of what the kernels do with them.  A plain module: no fixtures.

A probe layer is *exact* when every product w * x and the bias are integer
multiples of one power of two q and sum_k |w_kn x_k| + |b_n| <= 2^20 q for
every output (span_bits).  Then every partial sum, in any order, is
representable in fp32 -- with four bits to spare, so also in any accumulator at
least as wide as fp32 -- and the fp32 MFMA chain, the split-K sum, the split
GEMMs of bf16x6 / fp16x3 and a float64 forward that stores its activations as
fp32 all give the same bits.  All probes use identity scalers.

Families (the builders return a Probe):
  dyadic_model   A  relu / linear, weights +-1/2: activations of up to 16 bits
                    (the hi and mid activation planes of bf16x6) and the routing
                    of every k and every column
  sign_model     B  saturating tanh (+-1) or sigmoid (0 / 1) logic: routing at any
                    depth, in all three modes
  planes3_model  C  three-part weights (1 + 2^-9 + 2^-17) times one-part
                    activations (+-1): the low weight planes
  planes2_model  C  two-part weights times two-part activations (1 + 2^-8):
                    the mid * mid product of bf16x6
  planes1x3_model C one-part weights times three-part activations: the lo
                    activation plane, which no family A value of <= 16 bits has

Families C read a first layer of threshold units tanh(2048 (p_a - theta_i)) and
take the difference of two neighbours, which is 2 inside the band theta_i < p_a
< theta_i+1 and 0 outside: per point only a few columns carry a value, which is
what keeps the *output* layer's span under 20 bits although each value is 18
bits wide.
"""
from collections import namedtuple

import numpy as np

Probe = namedtuple("Probe", "name weights biases acts pts")

N_PTS = 611  # no multiple of 32; > two 256-point tiles; about ten 64-point tiles
ZERO3, ONE3, ZERO4, ONE4 = np.zeros(3), np.ones(3), np.zeros(4), np.ones(4)
IDENTITY = (ZERO3, ONE3, ZERO4, ONE4)  # x_mean, x_scale, y_mean, y_scale

# The products the split GEMMs keep, as (weight plane, activation plane), in the
# kernels' issue order (layer_gemm_x16 / layer_gemm_h16 in csrc/ik_ann_kernel.h).
BF16_KEPT = ((0, 2), (1, 1), (2, 0), (0, 1), (1, 0), (0, 0))
F16_KEPT = ((0, 1), (1, 0), (0, 0))


# ------------------------------------------------------------ references ----
def _activate(a, z):
    if a == "tanh":
        return np.tanh(z)
    if a == "relu":
        return np.maximum(z, 0)
    if a == "sigmoid":
        with np.errstate(over="ignore"):
            return 1 / (1 + np.exp(-z))
    if a != "linear":
        raise ValueError(a)
    return z


def forward_f64_stored_f32(weights, biases, acts, pts, start=0, h=None):
    """Float64 Dense layers with every layer's activations rounded to fp32, as
    the kernels' LDS and HBM tiles hold them.  Identity scalers.  With `h` (fp32
    activations entering layer `start`) only the layers from `start` on run."""
    if h is None:
        h = np.asarray(pts, np.float64).reshape(-1, 3).astype(np.float32)
    for W, b, a in zip(weights[start:], biases[start:], acts[start:]):
        z = h.astype(np.float64) @ np.asarray(W, np.float64) + np.asarray(b, np.float64)
        h = _activate(a, z).astype(np.float32)
    return h


def layer_inputs(probe):
    """The fp32 activations entering every layer (index l: the input of layer l)."""
    hs = [np.asarray(probe.pts, np.float64).astype(np.float32)]
    for l in range(len(probe.weights) - 1):
        hs.append(forward_f64_stored_f32(probe.weights[:l + 1], probe.biases, probe.acts, None,
                                         start=l, h=hs[-1]))
    return hs


def _low_exp(a):
    """Exponent of the lowest set bit of each float64 (a large number for 0)."""
    m, e = np.frexp(np.asarray(a, np.float64))
    mi = np.abs(m * 2.0 ** 53).astype(np.int64)
    low = (mi & -mi).astype(np.float64)
    tz = np.frexp(np.where(low > 0, low, 1.0))[1] - 1
    return np.where(mi != 0, e.astype(np.int64) - 53 + tz, 1 << 20)


def span_bits(probe, pts=None):
    """Per layer log2(max sum |terms| / q): q the largest power of two dividing
    every product w_kn x_pk and every bias of the layer, the sum over k plus
    |b_n|, the maximum over points and outputs.  From a float64 forward that
    stores fp32."""
    h = np.asarray(probe.pts if pts is None else pts, np.float64).astype(np.float32)
    out = []
    for W, b, a in zip(probe.weights, probe.biases, probe.acts):
        x, W64, b64 = h.astype(np.float64), np.asarray(W, np.float64), np.asarray(b, np.float64)
        # the lowest bit of an exact product is the sum of its factors' lowest bits
        qe = int((_low_exp(x).min(axis=0) + _low_exp(W64).min(axis=1)).min())
        qe = min(qe, int(_low_exp(b64).min()))
        tot = (np.abs(x) @ np.abs(W64) + np.abs(b64)).max()
        out.append(float(np.log2(tot)) - qe if tot > 0 else 0.0)
        h = _activate(a, x @ W64 + b64).astype(np.float32)
    return out


# ------------------------------------------------- the kernels' operand splits ----
def bf16_rne(x):
    """fp32 -> bf16 (round to nearest even) -> fp32, finite values."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    u = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return u.view(np.float32)


def bf16_split3(x):
    """x = hi + mid + lo in bf16: split3 on the device, bf16_split3 in ik_ann_pack.cpp."""
    x = np.asarray(x, np.float32)
    hi = bf16_rne(x)
    r1 = x - hi
    mid = bf16_rne(r1)
    return hi, mid, bf16_rne(r1 - mid)


def h_scale_exp(W):
    """ann_h_scale_exp: the power of two bringing max |w| to [2^13, 2^14)."""
    mx = float(np.abs(W).max())
    if not mx > 0 or not np.isfinite(mx):
        return 0
    return 14 - int(np.frexp(mx)[1])


def f16_split2(x):
    """x = hi + lo in fp16, each rounded to nearest (ann_pack_layer_h, store_h4)."""
    x = np.asarray(x, np.float32)
    hi = x.astype(np.float16).astype(np.float32)
    return hi, (x - hi).astype(np.float16).astype(np.float32)


def layer_kind(dims, acts, l, mode):
    """The arithmetic layer l runs in `mode` (AnnLayout in ik_ann_pack.cpp and
    ann_launch): "fp32", "bf16x6" or "fp16x3"."""
    big = len(dims) - 1 > 24 or max(dims) > 1024
    wide = max(dims) > 512
    splittable = (not wide or big) and l > 0 and (dims[l + 1] + 31) // 32 > 1
    if mode == "fp32" or not splittable:
        return "fp32"
    if big or mode == "bf16x6":
        return "bf16x6"
    return "fp16x3" if acts[l - 1] in ("tanh", "sigmoid") else "fp32"


def forward_emulated(probe, mode, drop=None, pts=None):
    """The forward with the split GEMMs restated plane by plane: a split layer's
    pre-activation is bias + the sum of the kept plane products (float64, exact
    for an exact probe), rounded to fp32.  drop: index into BF16_KEPT / F16_KEPT
    of a product to leave out of every split layer."""
    dims = [3] + [W.shape[1] for W in probe.weights]
    h = np.asarray(probe.pts if pts is None else pts, np.float64).astype(np.float32)
    for l, (W, b, a) in enumerate(zip(probe.weights, probe.biases, probe.acts)):
        kind = layer_kind(dims, probe.acts, l, mode)
        b64 = np.asarray(b, np.float64)
        if kind == "bf16x6":
            xp, wp = bf16_split3(h), bf16_split3(W)
            z = b64 + sum(xp[x].astype(np.float64) @ wp[w].astype(np.float64)
                          for i, (w, x) in enumerate(BF16_KEPT) if i != drop)
        elif kind == "fp16x3":
            s = h_scale_exp(W)
            xp, wp = f16_split2(h), f16_split2(np.ldexp(np.asarray(W, np.float32), s))
            acc = np.ldexp(b64, s) + sum(xp[x].astype(np.float64) @ wp[w].astype(np.float64)
                                         for i, (w, x) in enumerate(F16_KEPT) if i != drop)
            z = np.ldexp(acc.astype(np.float32).astype(np.float64), -s)
        else:
            z = h.astype(np.float64) @ np.asarray(W, np.float64) + b64
        h = _activate(a, z.astype(np.float32).astype(np.float64)).astype(np.float32)
    return h


# ------------------------------------------------------------ builders ----
def _cover(W, rng, mag):
    """Every k feeds some column: a row of W still empty gets +-mag in column
    k mod N.  Returns the number of sources per column."""
    K, N = W.shape
    for k in np.flatnonzero(~W.any(axis=1)):
        W[k, k % N] = mag * rng.choice([1.0, -1.0])
    return (W != 0).sum(axis=0)


def _sources(l, K, N, rng, n):
    """n distinct source rows per column: (7 j + l) mod K first, the rest random."""
    assert K > n
    k1 = (7 * np.arange(N) + l) % K
    o1 = 1 + rng.integers(0, K - 1, N)  # offsets from k1 in 1 .. K-1, distinct
    if n == 2:
        return np.stack([k1, (k1 + o1) % K])
    o2 = 1 + rng.integers(0, K - 2, N)
    o2 += o2 >= o1
    return np.stack([k1, (k1 + o1) % K, (k1 + o2) % K])


def dyadic_model(dims, seed=0, n=N_PTS):
    """Family A.  For at most 4 hidden layers: the span grows a bit per layer."""
    rng = np.random.default_rng(seed)
    L = len(dims) - 1
    Ws, bs, acts = [], [], []
    N = dims[1]
    W = np.zeros((3, N), np.float32)
    W[np.arange(N) % 3, np.arange(N)] = rng.choice([1.0, -1.0, 2.0, 0.5], N)
    Ws.append(W)
    bs.append(rng.integers(-4, 5, N).astype(np.float32))
    acts.append("linear")
    for l in range(1, L - 1):
        K, N = dims[l], dims[l + 1]
        W = np.zeros((K, N), np.float32)
        ks = _sources(l, K, N, rng, 2)
        W[ks[0], np.arange(N)] = 0.5
        W[ks[1], np.arange(N)] = rng.choice([0.5, -0.5], N)
        _cover(W, rng, 0.5)
        Ws.append(W)
        bs.append(rng.integers(-2, 3, N).astype(np.float32))
        acts.append("relu" if l % 2 else "linear")
    K = dims[L - 1]
    p2 = 1
    while p2 < K / 4:
        p2 *= 2
    W = np.zeros((K, 4), np.float32)
    W[np.arange(K), np.arange(K) % 4] = rng.choice([1.0, -1.0, 2.0, -2.0], K) / p2
    Ws.append(W)
    bs.append(np.zeros(4, np.float32))
    acts.append("linear")
    pts = rng.integers(-64, 65, (n, 3)) / 8.0
    return Probe(f"A{tuple(dims)}", Ws, bs, acts, pts)


def sign_model(dims, act="tanh", seed=0, n=N_PTS):
    """Family B.  tanh: activations +-1, every pre-activation an odd multiple of
    16.  sigmoid: activations 0 / 1, every pre-activation an odd multiple of 256,
    where the kernels' exp2 overflows to inf (the low side is an exact 0) or
    underflows to 0 (the high side an exact 1)."""
    rng = np.random.default_rng(seed)
    L = len(dims) - 1
    s0, s, half = (32.0, 16.0, 16.0) if act == "tanh" else (512.0, 512.0, 256.0)
    Ws, bs, acts = [], [], []
    N = dims[1]
    W = np.zeros((3, N), np.float32)
    W[np.arange(N) % 3, np.arange(N)] = s0 * rng.choice([1.0, -1.0], N)
    Ws.append(W)
    bs.append((s0 * rng.integers(-8, 8, N) + s0 / 2).astype(np.float32))
    acts.append(act)
    for l in range(1, L - 1):
        K, N = dims[l], dims[l + 1]
        W = np.zeros((K, N), np.float32)
        ks = _sources(l, K, N, rng, 3)
        for row in ks:
            W[row, np.arange(N)] = s * rng.choice([1.0, -1.0], N)
        cnt = _cover(W, rng, s)
        sign = rng.choice([1.0, -1.0], N)
        # an odd number of +-1 terms: the bias stands in for one
        b = np.where(cnt % 2 == 0, half * sign, 0.0)
        if act == "sigmoid":  # the same logic on u = 2 h - 1: 256 sum(s u) = 512 sum(s h) - 256 sum(s)
            b -= half * np.sign(W).sum(axis=0)
        Ws.append(W)
        bs.append(b.astype(np.float32))
        acts.append(act)
    K = dims[L - 1]
    W = np.zeros((K, 4), np.float32)
    # an integer in +-[1, 7] over a power of two that keeps |output| <= 4: the FK
    # round trip takes angles up to 2 pi
    p2 = 1
    while 4 * p2 < 7 * ((K + 3) // 4):
        p2 *= 2
    W[np.arange(K), np.arange(K) % 4] = rng.integers(1, 8, K) * rng.choice([1.0, -1.0], K) / p2
    Ws.append(W)
    bs.append(np.zeros(4, np.float32))
    acts.append("linear")
    pts = rng.integers(-8, 9, (n, 3)).astype(np.float64)
    return Probe(f"B-{act}{tuple(dims)}", Ws, bs, acts, pts)


def _band_units(N1, N2, mag, rng, n):
    """Layer 0: N1 threshold units tanh(2048 (p_a - theta)), a = u mod 3, theta =
    (t + 1/2) / 64 with the t of one axis distinct and rising; layer 1: column j
    is mag_j (unit i - unit i+1) of axis j mod 3, so 2 mag_j inside band i, else
    0.  Points: multiples of 1/64, per axis inside a random band or (one in
    eight) below every threshold."""
    W0, b0 = np.zeros((3, N1), np.float32), np.zeros(N1, np.float32)
    W1 = np.zeros((N1, N2), np.float32)
    pts = np.full((n, 3), -8.0)
    for a in range(3):
        units = np.arange(a, N1, 3)
        t = np.sort(rng.choice(960, len(units), replace=False)) - 480
        W0[a, units] = 2048.0
        b0[units] = -(32.0 * t + 16.0)  # -2048 theta
        cols = np.arange(a, N2, 3)
        band = np.arange(len(cols)) % (len(units) - 1)
        W1[units[band], cols] = mag[cols]
        W1[units[band + 1], cols] = -mag[cols]
        inside = rng.integers(0, min(len(units) - 1, len(cols)), n)  # a band some column reads
        pts[:, a] = np.where(rng.integers(0, 8, n) == 0, -8.0, (t[inside] + 1) / 64.0)
    return W0, b0, W1, pts


def _out_pm1(K, rng):
    W = np.zeros((K, 4), np.float32)
    W[np.arange(K), np.arange(K) % 4] = rng.choice([1.0, -1.0], K)
    return W


def planes3_model(dims, seed=0, n=N_PTS):
    """Family C, three-part weights times one-part activations: dims (3, N1, N2,
    4), N2 <= N1.  Layer 1's weights are s (1 + 2^-9 + 2^-17), s = +-1 on axis 0
    and +-1/2 on the others: bf16 parts 1, 2^-9, 2^-17; scaled by 2^13 the fp16
    parts are 8208 and 0.0625."""
    rng = np.random.default_rng(seed)
    _, N1, N2, _ = dims
    base = np.float32(1 + 2.0 ** -9 + 2.0 ** -17)
    mag = base * rng.choice([1.0, -1.0], N2) * np.where(np.arange(N2) % 3 == 0, 1.0, 0.5)
    W0, b0, W1, pts = _band_units(N1, N2, mag.astype(np.float32), rng, n)
    return Probe(f"C3{tuple(dims)}", [W0, W1, _out_pm1(N2, rng)],
                 [b0, np.zeros(N2, np.float32), np.zeros(4, np.float32)],
                 ["tanh", "linear", "linear"], pts)


def planes2_model(dims, seed=0, n=N_PTS, a=1 + 2.0 ** -8, w=1 + 2.0 ** -8, fam="C2"):
    """Family C, two-part times two-part: dims (3, N1, N2, N3, 4).  Layer 1
    turns the +-1 units into activations 0 or +-a, a = 1 + 2^-8 (bf16 hi 1, mid
    2^-8); layer 2's weights are +-w, w = 1 + 2^-8, two per column: hi*hi,
    hi*mid, mid*hi and mid*mid all occur, and no lo part exists to be dropped."""
    rng = np.random.default_rng(seed)
    _, N1, N2, N3, _ = dims
    a, w = np.float32(a), np.float32(w)
    mag = (a / 2) * rng.choice([1.0, -1.0], N2)
    W0, b0, W1, pts = _band_units(N1, N2, mag.astype(np.float32), rng, n)
    W2 = np.zeros((N2, N3), np.float32)
    k1 = (7 * np.arange(N3) + 2) % N2
    W2[k1, np.arange(N3)] = w * rng.choice([1.0, -1.0], N3)
    W2[(k1 + N2 // 2) % N2, np.arange(N3)] = w * rng.choice([1.0, -1.0], N3)
    return Probe(f"{fam}{tuple(dims)}", [W0, W1, W2, _out_pm1(N3, rng)],
                 [b0, np.zeros(N2, np.float32), np.zeros(N3, np.float32), np.zeros(4, np.float32)],
                 ["tanh", "linear", "linear", "linear"], pts)


def planes1x3_model(dims, seed=0, n=N_PTS):
    """Family C, one-part weights (+-1) times three-part activations (0 or +-(1 +
    2^-9 + 2^-17)): the activations' lo plane."""
    return planes2_model(dims, seed, n, a=1 + 2.0 ** -9 + 2.0 ** -17, w=1.0, fam="C1")


# ------------------------------------------------------------ the cases ----
DEEP = (3,) + (500,) * 12 + (4,)
THIRTY = (3,) + (64,) * 29 + (4,)
FUSED_DIMS = [(3, 100, 37, 250, 4), (3, 500, 500, 500, 500, 4), (3, 64, 32, 64, 4)]
WIDE_DIMS = [(3, 768, 500, 4), (3, 1024, 1024, 4)]
LAYERED_DIMS = [(3, 1100, 200, 37, 4), (3, 2048, 2048, 4)]

_BUILD = {"A": dyadic_model, "C1": planes1x3_model, "Bt": lambda d, **k: sign_model(d, "tanh", **k),
          "Bs": lambda d, **k: sign_model(d, "sigmoid", **k), "C3": planes3_model,
          "C2": planes2_model}


def _cases():
    c = {"fused": [], "wide": [], "layered": []}
    for path, dims_list, b_only in (("fused", FUSED_DIMS, DEEP), ("wide", WIDE_DIMS, None),
                                    ("layered", LAYERED_DIMS, THIRTY)):
        for d in dims_list:
            c[path] += [("A", d), ("Bt", d), ("Bs", d)]
        if b_only:
            c[path] += [("Bt", b_only), ("Bs", b_only)]
    # family C has its own shapes: N2 <= N1, and one more layer for the two-part probe
    c["fused"] += [("C1", (3, 128, 96, 64, 4)), ("C3", (3, 250, 100, 4)), ("C3", (3, 500, 500, 4)), ("C2", (3, 128, 96, 64, 4))]
    c["wide"] += [("C3", d) for d in WIDE_DIMS]
    c["layered"] += [("C1", (3, 1100, 200, 37, 4)), ("C3", (3, 2048, 2048, 4)), ("C2", (3, 1100, 200, 37, 4))]
    return c


CASES = _cases()
MODES = {"fused": ("fp32", "bf16x6", "fp16x3"), "wide": ("fp32", "bf16x6", "fp16x3"),
         "layered": ("fp32", "bf16x6", "fp16x3")}
# what ann_effective_mode() answers for a split request on each path
EFFECTIVE = {"wide": {"bf16x6": "fp32", "fp16x3": "fp32"},
             "layered": {"bf16x6": "bf16x6", "fp16x3": "bf16x6"}}


def case_id(case):
    fam, dims = case
    d = "x".join(str(v) for v in dims) if len(dims) <= 6 else f"{dims[1]}x{len(dims) - 2}"
    return f"{fam}-{d}"


_cache = {}


def build(case, n=N_PTS):
    """The Probe of a case (seeded by its dims; built once per process)."""
    key = (case, n)
    if key not in _cache:
        fam, dims = case
        _cache[key] = _BUILD[fam](dims, seed=len(dims) + dims[1], n=n)
    return _cache[key]


def expected(case):
    """(probe, expected fp32 output) of a case at N_PTS points."""
    key = (case, "exp")
    if key not in _cache:
        p = build(case)
        _cache[key] = forward_f64_stored_f32(p.weights, p.biases, p.acts, p.pts)
    return build(case), _cache[key]
