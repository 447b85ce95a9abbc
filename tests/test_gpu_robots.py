"""Every robot-dependent kernel on DH tables with no zero entry (tests/robots.py:
GEN_A, GEN_B, SKEW_DH) against the reference's golden outputs, the C oracle and
the numpy refine restatement: the FABRIK seed pose (seed_closed and
robot_const_kernel's P_k), the fused FK round trip (fk_error_cs) of the FABRIK,
ANN, refine and fused ANN + refine calls, the FK matrices, the refine Jacobian,
robots the reference rejects, and robot changes on one context.  On
SixDOFRobot's table most of that arithmetic multiplies by an exact 0 or 1;
tests/test_robots_cpu.py shows that here every table entry moves what these
tests bound by >= 1e6 x the bound, and that the seed's last bits cannot excuse
a count mismatch or a 1e-9 miss."""
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests import robots as RB
from tests.conftest import GOLDEN
from tests.test_gpu_ann_probes import _glorot_case, _load, _set_mode
from tests.test_gpu_refine import same, small_model, stats_match

pytestmark = pytest.mark.gpu

NAMES = list(RB.TABLES)
# the two benchmark configurations, and a solve of no iteration: the seed pose itself
FABRIK_CONFIGS = RB.CONFIGS + ((1e-3, 0),)
N_ANN = 2000


def _context(dh=None, **env):
    from inversekinematicsann_amd import _native
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        c = _native.Context(0)
    finally:
        for k in env:
            os.environ.pop(k, None)
    if dh is not None:
        c.set_robot(dh, RB.LINKS, RB.LIMITS)
    return c


@pytest.fixture(scope="module", params=[1, 0, 2], ids=["split", "simple", "split_refill1"])
def fab(request):
    """One context per FABRIK kernel variant (as tests/test_gpu_parity.py's ctx)."""
    c = _context(IKHIP_FABRIK_VARIANT=request.param)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx():
    c = _context()
    yield c
    c.close()


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "robots_general_dh.npz"), allow_pickle=False)


_oracle = {}


def oracle_fabrik(name, tol, mi):
    """O.fabrik_ikine on goals(dh), once per (table, configuration)."""
    key = (name, tol, mi)
    if key not in _oracle:
        dh = RB.TABLES[name]
        _oracle[key] = O.fabrik_ikine(RB.goals(dh), tol, mi, dh=dh, links=RB.LINKS)
    return _oracle[key]


def check_fabrik(got, ref, mi, what):
    """A fabrik_solve result against (angles, iters, joints, status) of the oracle or
    the golden: counts exact, NaN masks equal, angles and joints <= 1e-9, the first
    error and the iteration stats the reductions of the reference's rows."""
    ang, it, jo, st = got
    rang, rit, rjo, rst = ref
    n = len(rit)
    ok = rst == 0
    assert np.array_equal(it[ok], rit[ok]), (what, np.flatnonzero(it != rit)[:8].tolist())
    for a, r in ((ang, rang), (jo.reshape(n, 12), rjo.reshape(n, 12))):
        assert np.array_equal(np.isnan(a), np.isnan(r)), what
        fin = ~np.isnan(r)
        d = np.abs(a[fin] - r[fin]).max(initial=0.0)
        assert d <= 1e-9, (what, d)
    bad = np.flatnonzero(~ok)
    want = (int(bad[0]), int(rst[bad[0]])) if len(bad) else (-1, 0)
    assert (st.first_err, st.first_err_code) == want, what
    assert st.n_capped == int((rit[ok] >= mi).sum()), what
    assert st.sum_iters == int(rit[ok].sum()) and st.max_iters == int(rit[ok].max(initial=0)), what


# ------------------------------------------------------------- FABRIK ----
@pytest.mark.parametrize("name", NAMES)
def test_fabrik_against_oracle(fab, name):
    """6000 goals over all four quadrants and the seed's edge rows, every
    configuration twice (the second solve runs in the learned work order)."""
    dh = RB.TABLES[name]
    pts = RB.goals(dh)
    fab.set_robot(dh, RB.LINKS, RB.LIMITS)
    for tol, mi in FABRIK_CONFIGS:
        ref = oracle_fabrik(name, tol, mi)
        first = fab.fabrik_solve(pts, tol, mi, want_joints=True)
        again = fab.fabrik_solve(pts, tol, mi, want_joints=True)
        check_fabrik(first, ref, mi, (name, tol, mi))
        for a, b in zip(first[:3], again[:3]):
            assert same(a, b), (name, tol, mi)
        assert first[3].as_dict() == again[3].as_dict()
        assert first[3].first_oob == O.check_limits(pts, RB.LIMITS) == -1
        if mi == 0:
            assert not first[1].any()


@pytest.mark.parametrize("name", NAMES)
def test_fabrik_against_reference_golden(fab, golden, name):
    dh = RB.TABLES[name]
    pts = golden[f"{name}_points"]
    fab.set_robot(dh, RB.LINKS, RB.LIMITS)
    for k, (tol, mi) in enumerate(RB.CONFIGS):
        ref = tuple(golden[f"{name}_{f}_{k}"] for f in ("angles", "iters", "joints", "status"))
        for _ in range(2):
            got = fab.fabrik_solve(pts, tol, mi, want_joints=True)
            check_fabrik(got, ref, mi, (name, tol, mi))


@pytest.mark.parametrize("n", [1, 63, 65, 257])
def test_fabrik_ragged_sizes(fab, n):
    """The last n goals of GEN_A's set: the edge rows and, from 63 on, box rows."""
    dh = RB.GEN_A
    fab.set_robot(dh, RB.LINKS, RB.LIMITS)
    pts = RB.goals(dh)[-n:]
    for tol, mi in RB.CONFIGS:
        ref = tuple(a[-n:] for a in oracle_fabrik("GEN_A", tol, mi))
        check_fabrik(fab.fabrik_solve(pts, tol, mi, want_joints=True), ref, mi, (n, tol))


def test_fabrik_core_paths_bit_identical():
    """IKHIP_FABRIK_CORE 0 / 1 / 2 (general sqrt and division, the core sequences,
    those with the repeated distances taken once) give the same bits on GEN_A."""
    pts = RB.goals(RB.GEN_A)
    out = {}
    for core in (0, 1, 2):
        c = _context(RB.GEN_A, IKHIP_FABRIK_CORE=core)
        try:
            out[core] = [c.fabrik_solve(pts, tol, mi, want_joints=True) for tol, mi in RB.CONFIGS]
        finally:
            c.close()
    for core in (1, 2):
        for (a0, i0, j0, s0), (a1, i1, j1, s1) in zip(out[0], out[core]):
            assert same(i0, i1) and same(a0, a1) and same(j0, j1), core
            assert s0.as_dict() == s1.as_dict(), core


# --------------------------------------------------------- round trips ----
def check_round_trip(err, ang, pts, dh, what, bound=1e-12):
    """err against |O.fk(ang, dh) - p|: NaN exactly where the oracle's FK raises or
    the angles are NaN, within the bound elsewhere.  Returns the finite rows."""
    a64 = np.asarray(ang, np.float64)
    gone = np.isnan(a64).any(axis=1) | np.isnan(pts).any(axis=1)
    xyz, _, st = O.fk(np.where(gone[:, None], 0.0, a64), dh)
    gone |= st != 0
    assert np.array_equal(np.isnan(err), gone), what
    ref = np.linalg.norm(xyz[~gone] - pts[~gone], axis=1)
    d = np.abs(err[~gone] - ref).max()
    print(f"{what}: max |fk_err - oracle round trip| = {d:.3g} over {int((~gone).sum())} rows")
    assert d <= bound, (what, d)
    return ~gone


def check_fk_stats(st, err, fin, what):
    assert st.max_fk_err == err[fin].max(), what
    s = err[fin].sum()
    assert abs(st.sum_fk_err - s) <= 1e-12 * s, what


@pytest.mark.parametrize("name", NAMES)
def test_fabrik_round_trip(fab, name):
    dh = RB.TABLES[name]
    pts = RB.goals(dh)
    fab.set_robot(dh, RB.LINKS, RB.LIMITS)
    for tol, mi in RB.CONFIGS:
        ang, it, err, st = fab.fabrik_solve_fk(pts, tol, mi)
        ang2, it2, _, _ = fab.fabrik_solve(pts, tol, mi)
        assert same(ang, ang2) and same(it, it2)
        fin = check_round_trip(err, ang, pts, dh, f"fabrik {name} {tol:g}")
        check_fk_stats(st, err, fin, name)


@pytest.mark.parametrize("name", NAMES)
def test_refine_round_trip_and_parity(ctx, name):
    """ctx.refine on refine_fixture(dh) against refine_reference on the same table,
    by the criteria of tests/test_gpu_refine.py::test_parity_with_restatement, and
    its fk_err against the oracle's FK."""
    dh = RB.TABLES[name]
    p, seed, _ = RB.refine_fixture(dh)
    n = len(p)
    ctx.set_robot(dh, RB.LINKS, RB.LIMITS)
    for tol in (1e-6, 1e-9):
        ang, it, err, st = ctx.refine(p, seed, tol, 20, 1e-3, check_limits=False)
        rth, rit, _ = RB.refine_restated(dh, tol)
        assert st.n_capped == 0 and st.first_err == -1 and st.first_oob == -1
        assert (err <= tol).all()
        fin = check_round_trip(err, ang, p, dh, f"refine {name} {tol:g}")
        assert fin.all()
        check_fk_stats(st, err, fin, name)
        trip = np.linalg.norm(O.fk(ang, dh)[0] - p, axis=1)
        assert (trip <= tol + 1e-12).all()
        eq = it == rit
        d = np.abs(ang[eq] - rth[eq]).max()
        print(f"{name} tol {tol:g}: {int((~eq).sum())} of {n} step counts differ; max "
              f"|theta_gpu - theta_ref| = {d:.3g} (bound {RB.ANGLE_BOUND[name]:.3g})")
        assert eq.mean() >= 0.999 and (np.abs(it - rit) <= 1).all()
        assert d <= RB.ANGLE_BOUND[name]
        assert st.max_iters == it.max() and st.sum_iters == int(it.sum())


ANN_CASES = [("fused", "fp32"), ("fused", "fp16x3"), ("wide", "fp32"), ("layered", "fp32")]


@pytest.mark.parametrize("path,mode", ANN_CASES)
def test_ann_round_trip(ctx, monkeypatch, path, mode):
    """ann_solve's fk_err on the fused, wide and layered paths (the Glorot models of
    tests/test_gpu_ann_probes.py), and ann_solve_refined's two errors, on every table."""
    m, sc, _ = _glorot_case(path)
    _load(ctx, m.weights, m.biases, m.activations, sc)
    try:
        _set_mode(ctx, mode)
        for name, dh in RB.TABLES.items():
            pts = RB.goals(dh)[:N_ANN]
            ctx.set_robot(dh, RB.LINKS, RB.LIMITS)
            ang, err, st = ctx.ann_solve(pts, check_limits=False, want_fk_err=True)
            assert ang.dtype == np.float32 and np.isfinite(ang).all()
            fin = check_round_trip(err, ang, pts, dh, f"ann {path} {mode} {name}")
            assert fin.sum() > N_ANN // 2
            check_fk_stats(st, err, fin, (path, name))
            if path == "layered":  # several activation chunks per layer
                monkeypatch.setenv("IKHIP_ANN_ACT_MB", "1")
                ang2, err2, _ = ctx.ann_solve(pts, check_limits=False, want_fk_err=True)
                monkeypatch.delenv("IKHIP_ANN_ACT_MB")
                assert same(ang2, ang) and same(err2, err)
            if mode == "fp32":
                rang, rit, rerr, serr, rst = ctx.ann_solve_refined(
                    pts, 1e-6, 20, 1e-3, check_limits=False, want_seed_fk_err=True)
                assert same(serr, err)
                rfin = check_round_trip(rerr, rang, pts, dh, f"ann+refine {path} {name}")
                assert rfin.all() and np.abs(rang).max() <= np.pi
                check_fk_stats(rst, rerr, rfin, (path, name, "refined"))
                assert rst.n_capped == int((~(rerr <= 1e-6)).sum())
    finally:
        ctx.ann_set_mode("fp32")


@pytest.mark.parametrize("name", NAMES)
def test_fk_mats_against_reference_golden(ctx, golden, name):
    ctx.set_robot(RB.TABLES[name], RB.LINKS, RB.LIMITS)
    ang, ref = golden[f"{name}_fk_angles"], golden[f"{name}_fk_mats"]
    xyz, mats, st = ctx.fk(ang, with_mats=True)
    assert st.first_err == -1
    d = np.abs(mats - ref).max()
    print(f"{name}: max |mats - fkine| = {d:.3g}")
    assert d <= 1e-12 and np.abs(xyz - ref[:, 3, :3, 3]).max() <= 1e-12


# ------------------------------------------------------ rejected robots ----
def _small_ann(c):
    model, xs, ys = small_model()
    c.ann_load(model.weights, model.biases, model.activations, xs.mean, xs.scale, ys.mean,
               ys.scale)


def test_alpha_out_of_range_fails_every_row():
    """alpha_2 = 7 > 2 pi: the reference's FK raises for every angle row
    (forward.py:23-25), so does every FABRIK seed pose and every round trip."""
    dh = RB.with_entry(RB.GEN_A, 3, 1, 7.0)
    pts = RB.goals(RB.GEN_A)[:1000]
    p, seed, _ = RB.refine_fixture(RB.GEN_A)
    n = len(p)
    c = _context(dh)
    try:
        _small_ann(c)
        for tol, mi in RB.CONFIGS:
            ang, it, jo, st = c.fabrik_solve(pts, tol, mi, want_joints=True)
            assert (st.first_err, st.first_err_code) == (0, 4) and np.isnan(ang).all()
            assert (O.fabrik_ikine(pts, tol, mi, dh=dh)[3] == 4).all()
            _, _, err, st = c.fabrik_solve_fk(pts, tol, mi)
            assert (st.first_err, st.first_err_code) == (0, 4) and np.isnan(err).all()
        ang, it, err, st = c.refine(p, seed, 1e-6, 20, 1e-3, check_limits=False)
        assert np.isnan(err).all() and st.n_capped == n and not it.any()
        _, err, st = c.ann_solve(pts, check_limits=False, want_fk_err=True)
        assert np.isnan(err).all() and st.max_fk_err == 0.0 and st.sum_fk_err == 0.0
        _, _, err, serr, st = c.ann_solve_refined(pts, 1e-6, 20, 1e-3, check_limits=False,
                                                  want_seed_fk_err=True)
        assert np.isnan(err).all() and np.isnan(serr).all() and st.n_capped == len(pts)
        xyz, _, st = c.fk(seed)
        assert (st.first_err, st.first_err_code) == (0, 4) and np.isnan(xyz).all()
    finally:
        c.close()


def test_theta_out_of_range_fails_fabrik_alone():
    """theta_3 = 7: the seed pose's own FK raises for every goal (status 4), and the
    plan picks the simple kernel; FK of given angles and the ANN round trip never
    read the table's theta row and equal the oracle's."""
    dh = RB.with_entry(RB.GEN_A, 0, 2, 7.0)
    pts = RB.goals(RB.GEN_A)[:1000]
    _, seed, _ = RB.refine_fixture(RB.GEN_A)
    c = _context(dh)
    try:
        _small_ann(c)
        c.set_timing(True)
        for tol, mi in RB.CONFIGS:
            ang, it, jo, st = c.fabrik_solve(pts, tol, mi, want_joints=True)
            assert [k for k, _ in c.kernel_times()] == ["fabrik_simple_kernel"]
            assert (st.first_err, st.first_err_code) == (0, 4)
            assert np.isnan(ang).all()
            assert (O.fabrik_ikine(pts, tol, mi, dh=dh)[3] == 4).all()
        c.set_timing(False)
        xyz, _, st = c.fk(seed)
        rxyz, _, rst = O.fk(seed, dh)
        assert st.first_err == -1 and not rst.any() and np.abs(xyz - rxyz).max() <= 1e-12
        ang, err, st = c.ann_solve(pts, check_limits=False, want_fk_err=True)
        fin = check_round_trip(err, ang, pts, dh, "ann, theta_3 = 7")
        check_fk_stats(st, err, fin, "theta_3 = 7")
    finally:
        c.close()


def test_theta_1_is_not_read():
    """theta_1 = 7 in the table: every goal's own azimuth replaces it
    (inverse.py:123-125), so nothing changes and nothing is uploaded -- neither by
    the binding nor by ik_set_robot itself."""
    dh7 = RB.with_entry(RB.GEN_A, 0, 0, 7.0)
    pts = RB.goals(RB.GEN_A)
    c = _context(RB.GEN_A)
    try:
        want = c.fabrik_solve_fk(pts, 1e-3, 100)
        uploads = c.robot_uploads
        assert c.set_robot(dh7, RB.LINKS, RB.LIMITS) is False and c.robot_uploads == uploads
        flat = np.ascontiguousarray(dh7.reshape(16))
        assert c.lib.ik_set_robot(c.handle, flat.ctypes.data, None, None) == 0
        got = c.fabrik_solve_fk(pts, 1e-3, 100)
        for a, b in zip(want[:3], got[:3]):
            assert same(a, b)
        assert stats_match(want[3], got[3])
        fresh = _context(dh7)
        try:
            assert fresh.robot_uploads == 1
            got = fresh.fabrik_solve_fk(pts, 1e-3, 100)
            for a, b in zip(want[:3], got[:3]):
                assert same(a, b)
        finally:
            fresh.close()
    finally:
        c.close()


# ------------------------------------------- robot changes on one context ----
def _all_calls(c):
    pts = RB.goals(RB.GEN_A)[-1500:]
    p, seed, _ = RB.refine_fixture(RB.GEN_A)
    return (c.fabrik_solve_fk(pts, 1e-3, 100), c.refine(p[:1500], seed[:1500], 1e-6, 20, 1e-3),
            c.ann_solve(pts, check_limits=False, want_fk_err=True), c.fk(seed[:1500]))


def test_robot_changes_on_one_context():
    """One context, the ANN model loaded once before any set_robot, then GEN_A ->
    GEN_B -> GEN_A -> GEN_A with another alpha_3 -> another d_4 -> another theta_3:
    after each change every call gives the bits of a fresh context with that robot
    (FABRIK, refine and analytic read constants uploaded by ik_set_robot, the ANN
    paths rebuild theirs from the host's table at launch)."""
    steps = [RB.GEN_A, RB.GEN_B, RB.GEN_A, RB.with_entry(RB.GEN_A, 3, 2, -0.8),
             RB.with_entry(RB.GEN_A, 1, 3, 0.45), RB.with_entry(RB.GEN_A, 0, 2, 0.7)]
    c = _context()
    try:
        _small_ann(c)
        for i, dh in enumerate(steps):
            assert c.set_robot(dh, RB.LINKS, RB.LIMITS) is True
            got = _all_calls(c)
            fresh = _context(dh)
            try:
                _small_ann(fresh)
                want = _all_calls(fresh)
            finally:
                fresh.close()
            for call, (g, w) in enumerate(zip(got, want)):
                for a, b in zip(g[:-1], w[:-1]):
                    assert (a is None and b is None) or same(a, b), (i, call)
                assert stats_match(g[-1], w[-1]), (i, call, g[-1].as_dict(), w[-1].as_dict())
            # and the result is this robot's: the FABRIK round trip against the oracle
            ang, _, err, _ = got[0]
            check_round_trip(err, ang, RB.goals(RB.GEN_A)[-1500:], dh, f"step {i}")
    finally:
        c.close()
