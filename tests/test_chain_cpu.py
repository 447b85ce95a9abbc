"""ik_chain_solve without a GPU: the ABI's declaration against the binding, the row
header (csrc/ik_chain_row.h) in a stand-alone host program against the numpy
restatement (kinematics/chain.py) byte for byte, the restatement against
refine_reference at nj = 4, against an FK that shares nothing with it and against
long double, on the tables of tests/chain_fixtures.py; the restart fixtures; the
refusals of the Python entry points and of the command line.
tests/test_gpu_chain.py runs the same fixtures through the kernel."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import chain_fixtures as F
from tests.conftest import ROOT
from tests.robots import GEN_A, GEN_B, SIXDOF_DH, SKEW_DH, refine_fixture
from tests.test_refine_limits_cpu import (DH, FIXED, LIM, fixed_fixture, fixed_reference,
                                          limited_fixture, limited_reference)

CLANGXX = "/opt/rocm/llvm/bin/clang++"  # csrc/Makefile HOSTCXX
CSRC = os.path.join(ROOT, "inversekinematicsann_amd", "csrc")
SPECIAL = (0.0, np.pi, -np.pi, np.pi / 2, -np.pi / 2)


def same(a, b):
    return a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


# 1 ---------------------------------------------------------------------------
def test_declaration_and_binding_agree():
    import ctypes
    from inversekinematicsann_amd import _native
    hdr = open(os.path.join(ROOT, "include", "ikhip.h")).read()
    m = re.search(r"^int ik_chain_solve\(ik_ctx \*ctx,(.*?)\);", hdr, re.M | re.S)
    assert m and "ik_chain_solve" in _native.EXPORTED_SYMBOLS
    params = [p.strip() for p in
              ("ik_ctx *ctx," + re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)).split(",")]
    kind = {"ik_ctx *": ctypes.c_void_p, "const double *": ctypes.c_void_p,
            "double *": ctypes.c_void_p, "int32_t *": ctypes.c_void_p, "int64_t ": ctypes.c_int64,
            "int32_t ": ctypes.c_int32, "double ": ctypes.c_double, "int ": ctypes.c_int,
            "ik_stats *": ctypes.POINTER(_native.IkStats)}
    want = []
    for p in params:
        typ = re.match(r"(.*?)(\w+)$", p).group(1)
        want.append(kind[typ])
    got = _native.load_library().ik_chain_solve.argtypes
    assert len(got) == 18 and list(got) == want


# 2 ---------------------------------------------------------------------------
def _angle_rows(nj, rng, n):
    th = rng.uniform(-np.pi, np.pi, (n, nj))
    sp = np.array([[v] * nj for v in SPECIAL])
    one = rng.uniform(-np.pi, np.pi, (len(SPECIAL) * nj, nj))
    for k, v in enumerate(SPECIAL):
        for j in range(nj):
            one[nj * k + j, j] = v
    return np.concatenate([th, sp, one])


def _host_blocks():
    """Per nj = 2..8 a block under limits that bind and a block with every joint free:
    (the doubles the program reads, the doubles it has to write)."""
    from inversekinematicsann_amd.kinematics import chain as C
    blocks, want = [], []
    lam2 = np.float64(1e-3) * np.float64(1e-3)
    for nj in range(2, 9):
        dh = GEN_A if nj == 4 else F.table(nj)
        consts = C._consts(dh, np.float64)
        a, d, ca, sa, bad = consts
        assert not bad
        jc = np.zeros((8, 4))
        jc[:nj] = np.stack([a, d, ca, sa], axis=1)
        rng = np.random.default_rng(50 + nj)
        for limited_block in (True, False):
            lo, hi = np.full(8, -np.inf), np.full(8, np.inf)
            if limited_block:  # joint 1 free, joint 2 fixed, the others narrow
                lo[1:nj], hi[1:nj] = -0.6, 0.4
                lo[1] = hi[1] = 0.25
            limited = ~(np.isneginf(lo[:nj]) & np.isposinf(hi[:nj]))
            mask = int((limited << np.arange(nj)).sum())
            th = C._place(_angle_rows(nj, rng, 200), lo[:nj], hi[:nj], limited, np.float64)
            goal = C.chain_fk(dh, th + rng.normal(0, 0.3, th.shape)) + rng.normal(0, 0.01, (len(th), 3))
            s, c = np.sin(th), np.cos(th)
            (x, y, z), J = C._chain_cs(consts, s, c)
            e = (goal[:, 0] - x, goal[:, 1] - y, goal[:, 2] - z)
            if limited_block:
                dl, lock, rs = C._limited_step(J, e, lam2, th, lo[:nj], hi[:nj], limited)
                assert lock.any() and (nj == 2 or (rs >= 2).any())  # (nj 2: one limited joint)
            else:
                dl = C._solve(J, e, lam2, None)
                lock, rs = np.zeros((len(th), nj), bool), np.zeros(len(th))
            new = C._update(th, dl, lo[:nj], hi[:nj], limited, np.float64)
            cols = [x, y, z] + [col[k] for k in range(3) for col in J] + list(dl)
            cols += [(lock << np.arange(nj)).sum(axis=1).astype(np.float64), rs.astype(np.float64)]
            want.append(np.concatenate([np.stack(cols, axis=1), new], axis=1).ravel())
            blocks += [np.array([nj, len(th)], np.float64), np.asarray(dh, np.float64).ravel(),
                       jc.ravel(), lo, hi, np.array([mask, lam2]),
                       np.concatenate([th, s, c, goal], axis=1).ravel()]
    rows = np.concatenate([np.arange(1500), 2 ** 40 + np.arange(100), [2 ** 53 - 1]])
    tr = np.array([(r, a, j) for r in rows for a in (1, 2, 255) for j in (0, 3, 7)], np.float64)
    u = np.empty(len(tr))
    for a in (1, 2, 255):
        for j in (0, 3, 7):
            m = (tr[:, 1] == a) & (tr[:, 2] == j)
            u[m] = C.start_u(tr[m, 0].astype(np.uint64), a, j)
    assert len(u) > 4000 and u.min() >= 0 and u.max() < 1 and len(np.unique(u)) == len(u)
    data = np.concatenate([np.array([14.0])] + blocks + [np.array([float(len(tr))]), tr.ravel()])
    return data, np.concatenate(want + [u])


@pytest.mark.skipif(not os.path.exists(CLANGXX), reason="the ROCm clang++ is not installed")
def test_row_header_in_host_program(tmp_path):
    exe = os.path.join(str(tmp_path), "chain_row_check")
    subprocess.run([CLANGXX, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
                    "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", CSRC,
                    os.path.join(ROOT, "tests", "host", "chain_row_check.cpp"), "-o", exe],
                   check=True)
    data, want = _host_blocks()
    rows, out = tmp_path / "rows.f64", tmp_path / "out.f64"
    data.astype("<f8").tofile(rows)
    r = subprocess.run([exe, str(rows), str(out)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-4000:]
    assert "chain_row_check ok" in r.stdout, r.stdout[-4000:]
    got = np.fromfile(out, "<f8")
    assert got.shape == want.shape
    differ = np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))
    assert got.tobytes() == want.astype("<f8").tobytes(), (differ[:10], got[differ[:5]],
                                                          want[differ[:5]])


# 3 ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["SIXDOF_DH", "GEN_A", "GEN_B", "SKEW_DH"])
def test_four_joints_free_equals_refine_reference(name):
    from inversekinematicsann_amd.kinematics.chain import chain_refine_reference
    from inversekinematicsann_amd.kinematics.refine import refine_reference
    dh = {"SIXDOF_DH": SIXDOF_DH, "GEN_A": GEN_A, "GEN_B": GEN_B, "SKEW_DH": SKEW_DH}[name]
    if name == "SIXDOF_DH":
        from tests.test_refine_cpu import fixture
        p, seed, _ = fixture()
    else:
        p, seed, _ = refine_fixture(dh)
    for tol in (1e-6, 1e-9):
        want = refine_reference(p, seed, tol, 20, 1e-3, dh)
        th, it, tries, err = chain_refine_reference(p, seed, tol, 20, 1e-3, dh)
        assert same(th, want[0]) and same(it, want[1]) and same(err, want[2])
        assert not tries.any()


def test_four_joints_limited_equals_refine_reference():
    from inversekinematicsann_amd.kinematics.chain import chain_refine_reference
    cases = [(dh, sigma, 1e-9, 20) for dh in DH for sigma in (0.05, 0.3)] + [("sixdof", 0.05, 1e-6, 20)]
    for dh, sigma, tol, cap in cases:
        p, seed, _ = limited_fixture(dh, sigma)
        want = limited_reference(dh, sigma, tol, cap)
        th, it, tries, err = chain_refine_reference(p, seed, tol, cap, 1e-3, DH[dh], joint_limits=LIM)
        assert same(th, want[0]) and same(it, want[1]) and same(err, want[2]), (dh, sigma, tol)
    p, seed, _ = fixed_fixture()
    want = fixed_reference()
    th, it, tries, err = chain_refine_reference(p, seed, 1e-9, 30, 1e-3, SIXDOF_DH, joint_limits=FIXED)
    assert same(th, want[0]) and same(it, want[1]) and same(err, want[2])


# 4 ---------------------------------------------------------------------------
@pytest.mark.parametrize("nj", F.NJS)
def test_tables_have_no_zero_entry_and_converge_on_every_row(nj):
    dh = F.table(nj)
    assert dh.shape == (4, nj) and (dh != 0).all() and np.isfinite(dh).all()
    p, _, _ = F.chain_fixture(nj)
    for tol in F.TOLS:
        th, it, tries, err = F.restated(nj, tol)
        print(f"nj {nj} tol {tol:g}: steps max {it.max()}, mean {it.mean():.3f}; max err "
              f"{err.max():.3g}")
        assert (err <= tol).all() and it.max() <= F.MAX_ITER and not tries.any()
        assert np.abs(th).max() <= np.pi
        trip = np.linalg.norm((F.fk_longdouble(dh, th) - p).astype(np.float64), axis=1)
        assert trip.max() <= tol + 1e-12


# 5 ---------------------------------------------------------------------------
@pytest.mark.parametrize("nj", (2, 3, 4, 5, 6, 7, 8))
def test_chain_against_independent_fk_and_central_differences(nj):
    """The effector within 50 roundings of the chain's length of the long double
    product (and of the oracle's fk_n where it takes the table: 4 joints and more); the
    Jacobian within 1e-9 of central differences in long double with h = 1e-6
    (truncation h^2 / 6 L <= 2e-12, rounding 2^-64 L / h ~ 1e-12)."""
    from inversekinematicsann_amd.kinematics.chain import chain_fk, chain_jacobian
    from oracle import oracle as O
    dh = GEN_A if nj == 4 else F.table(nj)
    rng = np.random.default_rng(30 + nj)
    th = rng.uniform(-np.pi, np.pi, (256, nj))
    L = np.abs(dh[1]).sum() + np.abs(dh[2]).sum()
    got = chain_fk(dh, th)
    d = np.abs((got - F.fk_longdouble(dh, th)).astype(np.float64)).max()
    print(f"nj {nj}: max |FK - long double| = {d:.3g} (bound {50 * 2 ** -53 * L:.3g})")
    assert d <= 50 * 2 ** -53 * L
    if nj >= 4:
        ref = np.array([O.fk_n(dh, row)[-1][:3, 3] for row in th[:32]])
        assert np.abs(got[:32] - ref).max() <= 50 * 2 ** -53 * L
    J = chain_jacobian(dh, th)
    assert J.shape == (256, 3, nj) and not J[:, 2, 0].any()
    h = np.longdouble(1e-6)
    for i in range(nj):
        e = np.zeros(nj, np.longdouble)
        e[i] = h
        fd = (F.fk_longdouble(dh, th + e) - F.fk_longdouble(dh, th - e)) / (2 * h)
        assert np.abs((J[:, :, i] - fd).astype(np.float64)).max() <= 1e-9


# 6 ---------------------------------------------------------------------------
@pytest.mark.parametrize("nj", F.NJS)
def test_restatement_float64_against_long_double(nj):
    for k, tol in enumerate(F.TOLS):
        t64, i64, _, _ = F.restated(nj, tol)
        tld, ild, _, _ = F.restated(nj, tol, np.longdouble)
        eq = i64 == ild
        d = np.abs(t64[eq] - tld[eq].astype(np.float64)).max()
        print(f"nj {nj} tol {tol:g}: {int((~eq).sum())} rows differ in steps; max |dtheta| = "
              f"{d:.3g} (written {F.MEASURED_F64_VS_LONGDOUBLE[nj][k]:.3g})")
        assert (np.abs(i64 - ild) <= 1).all() and eq.mean() >= 0.999
        assert d <= F.MEASURED_F64_VS_LONGDOUBLE[nj][k]
    assert F.ANGLE_BOUND[nj] == 10 * max(F.MEASURED_F64_VS_LONGDOUBLE[nj])


def test_limited_restatement_float64_against_long_double():
    lo, hi = F.LIMITS6
    t64, i64, _, e64 = F.restated_limited6()
    tld, ild, _, _ = F.restated_limited6(np.longdouble)
    eq = i64 == ild
    d = np.abs(t64[eq] - tld[eq].astype(np.float64)).max()
    on = (t64 == lo) | (t64 == hi)
    print(f"{int((~eq).sum())} rows differ in steps; max |dtheta| = {d:.3g}; "
          f"{int(on.any(axis=1).sum())} rows end on a limit")
    assert (e64 <= 1e-9).all() and ((t64 >= lo) & (t64 <= hi)).all() and on.any()
    assert (np.abs(i64 - ild) <= 1).all() and eq.mean() >= 0.999
    assert d <= F.MEASURED_LIMITED6_F64_VS_LONGDOUBLE
    assert F.LIMITED6_ANGLE_BOUND == 10 * F.MEASURED_LIMITED6_F64_VS_LONGDOUBLE


# 7 ---------------------------------------------------------------------------
@pytest.mark.parametrize("nj", F.HOME_NJS)
def test_restarts_reduce_capped(nj):
    from inversekinematicsann_amd.kinematics.chain import chain_refine_reference
    p = F.home_fixture(nj)
    th0, it0, tr0, e0 = F.home_restated(nj, 0)
    th, it, tr, e = F.home_restated(nj, F.HOME_RESTARTS)
    capped = (int((~(e0 <= 1e-6)).sum()), int((~(e <= 1e-6)).sum()))
    print(f"nj {nj}: capped {capped}, attempts returned {np.bincount(tr)}")
    assert capped == F.HOME_CAPPED[nj] and capped[1] < capped[0]
    assert not tr0.any() and tr.max() <= F.HOME_RESTARTS
    # a row attempt 0 solves is attempt 0's; the others ran every attempt they needed
    done0 = e0 <= 1e-6
    assert same(th[done0], th0[done0]) and not tr[done0].any() and same(it[done0], it0[done0])
    assert (it[~done0] > it0[~done0]).all() and (e <= e0).all()
    # an explicit tiled home pose is the NULL seed
    again = chain_refine_reference(p, np.tile(F.table(nj)[0], (len(p), 1)), 1e-6, F.HOME_ITER[nj],
                                   F.DAMPING, F.table(nj), restarts=F.HOME_RESTARTS)
    assert all(same(a, b) for a, b in zip(again, (th, it, tr, e)))


def test_restart_starts_and_edge_rows():
    from inversekinematicsann_amd.kinematics import chain as C
    dh = F.table(5)
    p, sd, _ = F.chain_fixture(5)
    lim = [None, (-0.5, 0.25), None, (0.1, 0.1), None]
    # no step: the result is a placed start point, the best of the attempts' errors
    th, it, tr, e = C.chain_refine_reference(p[:300], sd[:300], 1e-9, 0, 1e-3, dh, lim, restarts=3)
    assert not it.any() and tr.max() == 3 and (np.bincount(tr) > 0).all()
    lo, hi = C.chain_limit_arrays(lim, 5)
    for a in range(4):
        rows = np.flatnonzero(tr == a)
        if a == 0:
            want = C._place(sd[rows], lo, hi, np.isfinite(lo), np.float64)
        else:
            u = np.stack([C.start_u(rows, a, j) for j in range(5)], axis=1)
            slo, shi = np.where(np.isfinite(lo), lo, -np.pi), np.where(np.isfinite(hi), hi, np.pi)
            want = slo + u * (shi - slo)
            assert (want[:, 3] == 0.1).all() and (np.abs(want) <= np.pi).all()
        assert same(th[rows], want)
    # a NaN goal: no step, no restart, the placed seed; its neighbours as alone
    q = p[:4].copy()
    q[1, 0] = np.nan
    th, it, tr, e = C.chain_refine_reference(q, sd[:4] + 7.0, 1e-9, 30, 1e-3, dh, restarts=3)
    assert it[1] == 0 and tr[1] == 0 and np.isnan(e[1]) and same(th[1], C.wrap(sd[1] + 7.0))
    alone = C.chain_refine_reference(p[:4], sd[:4] + 7.0, 1e-9, 30, 1e-3, dh, restarts=3)
    assert all(same(a[[0, 2, 3]], b[[0, 2, 3]]) for a, b in zip((th, it, tr, e), alone))
    # out of reach: every attempt runs, finite angles
    th, it, tr, e = C.chain_refine_reference([[50.0, 0.0, 0.0]], None, 1e-6, 10, 1e-3, dh, restarts=2)
    assert it[0] == 30 and e[0] > 1e-6 and np.isfinite(th).all()
    # some |alpha| > 2 pi: every error NaN, no step
    bad = np.array(dh)
    bad[3, 2] = 7.0
    th, it, tr, e = C.chain_refine_reference(p[:8], sd[:8], 1e-6, 10, 1e-3, bad, restarts=2)
    assert not it.any() and not tr.any() and np.isnan(e).all() and same(th, C.wrap(sd[:8]))


# 8 ---------------------------------------------------------------------------
def test_limit_parsing_refuses_what_the_library_refuses():
    from inversekinematicsann_amd.kinematics.chain import chain_dh, chain_limit_arrays
    ok = [(-1.0, 1.0)] * 6
    for i, bad, word in ((0, (np.nan, 1.0), "NaN"), (1, (1.0, -1.0), "lo > hi"),
                         (4, (-4.0, 1.0), "outside"), (5, (0.0, 3.2), "outside"),
                         (3, (-np.inf, 1.0), "infinite"), (0, (0.0, np.inf), "infinite")):
        jl = list(ok)
        jl[i] = bad
        with pytest.raises(ValueError, match=rf"joint {i + 1}: .*{word}"):
            chain_limit_arrays(jl, 6)
    with pytest.raises(ValueError, match="6 entries"):
        chain_limit_arrays(ok[:5], 6)
    lo, hi = chain_limit_arrays([None, (0.25, 0.25), (-np.pi, np.pi)], 3)
    assert np.array_equal(lo, [-np.inf, 0.25, -np.pi]) and np.array_equal(hi, [np.inf, 0.25, np.pi])
    lo, hi = chain_limit_arrays((np.full(5, -1.0), np.full(5, 1.0)), 5)
    assert (lo == -1).all() and (hi == 1).all()
    for nj in (1, 9):
        with pytest.raises(ValueError, match="not built"):
            chain_dh(np.ones((4, nj)))
    with pytest.raises(ValueError, match="non-finite"):
        chain_dh([[0, 0], [1, np.inf], [1, 1], [0, 0]])
    assert chain_dh([[np.nan, 0], [1, 1], [1, 1], [0, 0]]).shape == (4, 2)  # (theta: a seed)


def test_python_entry_points_refuse_without_a_gpu(monkeypatch):
    """The refusals come before the library is loaded or a context made."""
    from inversekinematicsann_amd import _native
    from inversekinematicsann_amd.kinematics.chain import ChainInverseKinematics

    def no_library(*a, **k):
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_native, "load_library", no_library)
    monkeypatch.setattr(_native, "context", no_library)
    ctx = object.__new__(_native.Context)  # (no ik_ctx_create)
    ctx.handle = None
    pts = np.zeros((3, 3))
    dh6 = F.table(6)
    for kw, word in (({"dh": np.ones((4, 1))}, "not built"), ({"dh": np.ones((4, 9))}, "not built"),
                     ({"joint_limits": (np.zeros(6), None)}, "both"),
                     ({"joint_limits": (None, np.zeros(6))}, "both"),
                     ({"restarts": 256}, "restarts"), ({"restarts": -1}, "restarts"),
                     ({"max_iter": -1}, "max_iter"),
                     ({"max_iter": 2 ** 31 - 1, "restarts": 1}, r"max_iter \* \(restarts \+ 1\)"),
                     ({"max_iter": 2 ** 23, "restarts": 255}, r"max_iter \* \(restarts \+ 1\)")):
        args = {"dh": dh6, "pts": pts, **kw}
        with pytest.raises(ValueError, match=word):
            ctx.chain_solve(**args)
        with pytest.raises(ValueError, match=word):
            ctx.chain_solve_device(ang=None, **args)
    for kw, word in (({"dh_matrix": np.ones((4, 1))}, "not built"),
                     ({"dh_matrix": np.ones((4, 9))}, "not built"), ({"restarts": 256}, "restarts"),
                     ({"joint_limits": [(1.0, 0.5)] + [None] * 5}, "joint 1: lo > hi"),
                     ({"damping": 0.0}, "damping")):
        with pytest.raises(ValueError, match=word):
            ChainInverseKinematics(**{"dh_matrix": dh6, **kw})
    ik = ChainInverseKinematics(dh6, [None] * 6)
    assert ik.joint_limits is None and ik.nj == 6 and ik.ikine([]) == []


def test_limit_forms_are_told_apart_by_type_also_at_two_joints(monkeypatch):
    """What reaches ik_chain_solve (the output of Context._chain_args) for every spelling
    of the limits, at nj = 2 -- where a pair and two entries have the same length -- and
    at nj = 3; through the class, which keeps a pair of arrays."""
    from inversekinematicsann_amd import _native
    from inversekinematicsann_amd.kinematics.chain import (ChainInverseKinematics,
                                                           chain_limit_arrays)
    inf = np.inf
    args = _native.Context._chain_args

    def reach(dh, jl):
        d, lo, hi = args(dh, jl, 60, 4)
        assert lo.dtype == hi.dtype == np.float64 and lo.flags.c_contiguous and hi.flags.c_contiguous
        return lo.tolist(), hi.tolist()

    dh2 = F.table(2)
    entries = [(-1.0, 1.0), (-0.5, 0.75)]
    want = ([-1.0, -0.5], [1.0, 0.75])
    assert reach(dh2, entries) == want
    assert reach(dh2, [list(e) for e in entries]) == want
    assert reach(dh2, (np.array(want[0]), np.array(want[1]))) == want     # the pair: arrays
    assert reach(dh2, [None, (-1.0, 1.0)]) == ([-inf, -1.0], [inf, 1.0])
    assert reach(dh2, [(-1.0, 1.0), None]) == ([-1.0, -inf], [1.0, inf])
    assert reach(dh2, [(-1.0, 1.0), (-1.0, 1.0)]) == ([-1.0, -1.0], [1.0, 1.0])
    assert args(dh2, None, 60, 4)[1:] == (None, None)
    for bad, word in (((np.array(want[0]), None), "both"), ((None, np.array(want[1])), "both"),
                      ((np.zeros(3), np.ones(3)), "2 entries"),
                      ((np.array(want[0]), (1.0, 0.75)), "both"),
                      ([(1.0, -1.0), None], "joint 1: lo > hi")):
        with pytest.raises(ValueError, match=word):
            args(dh2, bad, 60, 4)
    # the class keeps the pair and hands it over: the same arrays reach the library
    seen = {}

    class Ctx:
        def chain_solve(self, dh, pts, seed, joint_limits, *a):
            seen["limits"] = reach(dh, joint_limits)
            n = len(pts)
            return (np.zeros((n, dh.shape[1])), np.zeros(n, np.int32), np.zeros(n, np.int32),
                    np.zeros(n), _native.IkStats(first_err=-1))
    monkeypatch.setattr(_native, "context", lambda: Ctx())
    for dh, jl, lo, hi in ((dh2, entries, *want), (dh2, [None, (-1.0, 1.0)], [-inf, -1.0], [inf, 1.0]),
                           (dh2, (np.array(want[0]), np.array(want[1])), *want),
                           (F.table(3), [(-1.0, 1.0), None, (0.25, 0.25)], [-1.0, -inf, 0.25],
                            [1.0, inf, 0.25])):
        ik = ChainInverseKinematics(dh, jl)
        assert ik.ikine([[0.5, 0.5, 0.5]]) == [[0.0] * dh.shape[1]]
        assert seen.pop("limits") == (lo, hi)
        assert [a.tolist() for a in ik.joint_limits] == [lo, hi]
    # at nj = 3 a list of two arrays is still the pair, a list of three tuples the entries
    assert reach(F.table(3), [np.full(3, -1.0), np.full(3, 1.0)]) == ([-1.0] * 3, [1.0] * 3)
    with pytest.raises(ValueError, match="tuple or list"):
        chain_limit_arrays([np.array([-1.0, 1.0])] * 3, 3)


HIPCC = "/opt/rocm/bin/hipcc"  # csrc/Makefile HIPCC


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="the ROCm hipcc is not installed")
def test_no_chain_kernel_uses_scratch(tmp_path):
    """The limited kernels keep scalar state in lanes of VGPRs and the NJ = 8 one fills
    the 256 registers of two waves per SIMD: what the compiler reports for each of the 14
    instantiations, built with the Makefile's flags, has no scratch and no spilled VGPR."""
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                        "-ffp-contract=off", "-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(CSRC, "ik_chain.hip"), "-o", str(tmp_path / "ik_chain.o")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    names = re.findall(r"Function Name: \w*chain_solve_kernelILi(\d)ELb([01])E", r.stdout)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stdout)]
    spilled = [int(v) for v in re.findall(r"VGPRs Spill: (\d+)", r.stdout)]
    assert sorted(names) == sorted((str(nj), b) for nj in range(2, 9) for b in "01"), names
    assert len(scratch) == len(spilled) == 14
    assert not any(scratch) and not any(spilled), (names, scratch, spilled)


def cli_error(argv, capsys):
    from inversekinematicsann_amd.cli import main
    with pytest.raises(SystemExit) as ei:
        main(argv)
    assert ei.value.code == 2
    return capsys.readouterr().err


def test_cli_usage_errors(tmp_path, capsys):
    pts = tmp_path / "p.csv"
    pts.write_text("x,y,z\n1.0,0.5,0.2\n")
    dh = tmp_path / "dh.csv"
    np.savetxt(dh, F.table(3), delimiter=",")
    base = ["--inverse-kine", "--points", str(pts)]
    chain = base + ["--method", "chain"]
    assert "required: --dh" in cli_error(chain, capsys)
    assert "--dh is only valid with --method chain" in \
        cli_error(base + ["--method", "fabrik", "--dh", str(dh)], capsys)
    assert "--restarts is only valid with --method chain" in \
        cli_error(base + ["--method", "analytic", "--restarts", "2"], capsys)
    chain += ["--dh", str(dh)]
    assert "3 comma-separated fields" in cli_error(chain + ["--joint-limits=-1:1,,,"], capsys)
    assert "joint 2: lo > hi" in cli_error(chain + ["--joint-limits=,1:-1,"], capsys)
    assert "joint 3: a bound lies outside" in cli_error(chain + ["--joint-limits=,,0:3.2"], capsys)
    assert "--restarts takes 0..255" in cli_error(chain + ["--restarts", "256"], capsys)
    assert "not both" in cli_error(chain + ["--tol", "1e-6", "--refine-tol", "1e-6"], capsys)
    assert "--model is not valid" in cli_error(chain + ["--model", "m.h5"], capsys)
    one = tmp_path / "one.csv"
    np.savetxt(one, np.ones((4, 1)), delimiter=",")
    assert "not built" in cli_error(base + ["--method", "chain", "--dh", str(one)], capsys)
    seeds = tmp_path / "s.csv"
    seeds.write_text("theta1,theta2\n0.1,0.2\n")
    assert "--seed-angles: 1 rows of 2 angles" in \
        cli_error(chain + ["--seed-angles", str(seeds)], capsys)
