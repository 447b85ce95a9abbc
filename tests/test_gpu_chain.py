"""ik_chain_solve on the GPU: chain_solve_kernel<NJ, kLimited> against ik_refine bit for
bit at nj = 4, against the numpy restatement (kinematics/chain.py) on the tables of
tests/chain_fixtures.py for nj = 2, 3, 5, 6, 7, 8, under limits, with restarts, on edge
rows, through device pointers, its refusals, and the class and command line on top."""
import ctypes

import numpy as np
import pytest

from tests import chain_fixtures as F
from tests.robots import GEN_A, SIXDOF_DH, SKEW_DH, refine_fixture
from tests.test_gpu_refine import same
from tests.test_refine_limits_cpu import LIM, limited_fixture

pytestmark = pytest.mark.gpu

T4 = {"SIXDOF_DH": SIXDOF_DH, "GEN_A": GEN_A, "SKEW_DH": SKEW_DH}


@pytest.fixture(scope="module")
def ctx():
    from inversekinematicsann_amd import _native
    c = _native.Context(0)
    yield c
    c.set_joint_limits(None)
    c.set_robot(SIXDOF_DH)
    c.close()


def stats_equal(a, b, skip=("first_oob", "first_err", "first_err_code")):
    """Equal stats apart from `skip`; the FK-error sum is a float64 atomic sum whose order
    is free."""
    a, b = a.as_dict(), b.as_dict()
    for k in skip:
        a.pop(k), b.pop(k)
    sa, sb = a.pop("sum_fk_err"), b.pop("sum_fk_err")
    return a == b and abs(sa - sb) <= 1e-12 * max(abs(sa), abs(sb))


def stats_are_sums(st, it, err, tol):
    n = len(it)
    capped = ~(err <= tol)
    fin = np.isfinite(err)
    first = np.flatnonzero(capped & fin)
    assert st.first_oob == -1
    assert st.max_iters == (int(it.max()) if n else 0) and st.sum_iters == int(it.sum())
    assert st.n_capped == int(capped.sum())
    assert st.first_err == (int(first[0]) if len(first) else -1)
    assert st.first_err_code == (1 if len(first) else 0)
    assert st.max_fk_err == (err[fin].max() if fin.any() else 0.0)
    assert abs(st.sum_fk_err - err[fin].sum()) <= 1e-12 * max(n, 1)


def round_trip(dh, ang, p):
    return np.linalg.norm((F.fk_longdouble(dh, ang) - p).astype(np.float64), axis=1)


def four_joint_data(name):
    if name == "SIXDOF_DH":
        from tests.test_refine_cpu import fixture
        return fixture()[:2]
    return refine_fixture(T4[name])[:2]


# 1 ---------------------------------------------------------------------------
@pytest.mark.parametrize("limits", [None, LIM], ids=["free", "limited"])
@pytest.mark.parametrize("name", list(T4))
def test_four_joints_give_ik_refine_bits(ctx, name, limits):
    """Fails on a wrong sum order, a wrong column index or a lost lock."""
    dh = T4[name]
    p, seed = four_joint_data(name)
    if limits is not None and name == "SIXDOF_DH":  # seeds 0.3 rad off: joints lock in pairs
        p, seed, _ = limited_fixture("sixdof", 0.3)
    ctx.set_robot(dh)
    ctx.set_joint_limits(limits)
    try:
        for tol in (1e-6, 1e-9):
            want = ctx.refine(p, seed, tol, 20, 1e-3, check_limits=False)
            ang, it, tries, err, st = ctx.chain_solve(dh, p, seed, limits, tol, 20, 1e-3, 0)
            assert same(ang, want[0]) and same(it, want[1]) and same(err, want[2])
            assert tries.dtype == np.int32 and not tries.any()
            assert stats_equal(st, want[3])
            stats_are_sums(st, it, err, tol)
            if limits is not None:
                on = (ang == limits[0]) | (ang == limits[1])
                assert on.any() and ((ang >= limits[0]) & (ang <= limits[1])).all()
        for n in (0, 1, 63, 64, 65, 257):  # prefixes of the tol 1e-9 batch
            a, i, t, e, s = ctx.chain_solve(dh, p[:n], seed[:n], limits, 1e-9, 20, 1e-3, 0)
            assert a.shape == (n, 4) and i.shape == t.shape == e.shape == (n,)
            assert same(a, ang[:n]) and same(i, it[:n]) and same(e, err[:n]) and not t.any()
            stats_are_sums(s, i, e, 1e-9)
    finally:
        ctx.set_joint_limits(None)
        ctx.set_robot(SIXDOF_DH)


# 2, 3 ------------------------------------------------------------------------
@pytest.mark.parametrize("tol", F.TOLS)
@pytest.mark.parametrize("nj", F.NJS)
def test_parity_with_restatement(ctx, nj, tol):
    dh = F.table(nj)
    p, seed, _ = F.chain_fixture(nj)
    ang, it, tries, err, st = ctx.chain_solve(dh, p, seed, None, tol, F.MAX_ITER, F.DAMPING, 0)
    rth, rit, _, _ = F.restated(nj, tol)
    assert st.n_capped == 0 and st.first_err == -1 and (err <= tol).all() and not tries.any()
    eq = it == rit
    d = np.abs(ang[eq] - rth[eq]).max()
    trip = round_trip(dh, ang, p)
    print(f"nj {nj} tol {tol:g}: {int((~eq).sum())} of {len(p)} rows differ in steps; max "
          f"{it.max()}, mean {it.mean():.3f}; max |theta_gpu - theta_ref| on equal-count rows "
          f"= {d:.3g} (bound {F.ANGLE_BOUND[nj]:.3g}); max fk_err {err.max():.3g}, max long "
          f"double round trip {trip.max():.3g}")
    assert eq.mean() >= 0.999 and (np.abs(it - rit) <= 1).all()
    assert d <= F.ANGLE_BOUND[nj]
    assert (trip <= tol + 1e-12).all()
    if nj >= 4:  # the oracle's FK takes the table
        from oracle import oracle as O
        ref = np.array([O.fk_n(dh, row)[-1][:3, 3] for row in ang[:16]])
        assert (np.linalg.norm(ref - p[:16], axis=1) <= tol + 1e-12).all()
    stats_are_sums(st, it, err, tol)


# 4 ---------------------------------------------------------------------------
def test_limits_that_bind_at_six_joints(ctx):
    dh = F.table(6)
    p, seed, _ = F.chain_fixture(6)
    inf = np.inf
    lo, hi = F.LIMITS6  # the goals' angles lie inside: reachable; seeds 0.05 rad off start outside
    free = ctx.chain_solve(dh, p, seed, None, 1e-9, F.MAX_ITER, F.DAMPING, 0)
    ang, it, tries, err, st = ctx.chain_solve(dh, p, seed, (lo, hi), 1e-9, F.MAX_ITER, F.DAMPING, 0)
    on = (ang == lo) | (ang == hi)
    conv = err <= 1e-9
    print(f"{int(on.any(axis=1).sum())} rows end on a limit; {int((~conv).sum())} not converged; "
          f"the free solve leaves {int(((free[0] < lo) | (free[0] > hi)).any(axis=1).sum())} "
          "rows outside")
    assert ((ang >= lo) & (ang <= hi)).all() and on.any() and not same(ang, free[0])
    assert ((free[0] < lo) | (free[0] > hi)).any()
    assert conv.mean() >= 0.99 and (round_trip(dh, ang, p)[conv] <= 1e-9 + 1e-12).all()
    stats_are_sums(st, it, err, 1e-9)
    # against the restatement, as without limits: a lost lock moves an angle
    rth, rit, _, rerr = F.restated_limited6()
    eq = it == rit
    d = np.abs(ang[eq] - rth[eq]).max()
    print(f"{int((~eq).sum())} rows differ in steps from the restatement; max |theta_gpu - "
          f"theta_ref| on equal-count rows = {d:.3g} (bound {F.LIMITED6_ANGLE_BOUND:.3g}); max "
          f"|err_gpu - err_ref| = {np.abs(err - rerr)[eq].max():.3g}")
    assert eq.mean() >= 0.999 and (np.abs(it - rit) <= 1).all() and st.n_capped == 0
    assert d <= F.LIMITED6_ANGLE_BOUND
    assert np.array_equal(on[eq], ((rth == lo) | (rth == hi))[eq])
    # every joint free, spelled as arrays: the bits of passing NULL; never-binding limits too
    for jl in ((np.full(6, -inf), np.full(6, inf)), (np.full(6, -np.pi), np.full(6, np.pi))):
        got = ctx.chain_solve(dh, p, seed, jl, 1e-9, F.MAX_ITER, F.DAMPING, 0)
        assert all(same(g, w) for g, w in zip(got[:4], free[:4])) and stats_equal(got[4], free[4], ())
    # lo == hi holds a joint
    lo2, hi2 = lo.copy(), hi.copy()
    lo2[3] = hi2[3] = 0.25
    ang, it, tries, err, st = ctx.chain_solve(dh, p, seed, (lo2, hi2), 1e-6, F.MAX_ITER, F.DAMPING, 0)
    assert ang[:, 3].tobytes() == np.full(len(ang), 0.25).tobytes()
    assert ((ang >= lo2) & (ang <= hi2)).all() and np.isfinite(ang).all()


# 5 ---------------------------------------------------------------------------
def test_restart_start_points(ctx):
    """No step is taken, so a row's angles are a placed start point: equal bit for bit
    wherever the kernel and the restatement return the same attempt."""
    from inversekinematicsann_amd.kinematics.chain import chain_refine_reference
    for nj, lim, seeded in ((5, [None, (-0.5, 0.25), None, (0.1, 0.1), None], True),
                            (6, None, False)):  # (the home pose, far from most goals)
        dh = F.table(nj)
        p, seed, _ = F.chain_fixture(nj)
        seed = seed if seeded else None
        ang, it, tries, err, st = ctx.chain_solve(dh, p, seed, lim, 1e-9, 0, F.DAMPING, 3)
        rth, rit, rtr, rerr = chain_refine_reference(p, seed, 1e-9, 0, F.DAMPING, dh, lim, restarts=3)
        agree = tries == rtr
        print(f"nj {nj}: attempts returned {np.bincount(tries, minlength=4)}, "
              f"{int((~agree).sum())} rows differ from the restatement")
        assert agree.mean() >= 0.999 and same(ang[agree], rth[agree])
        assert not it.any() and st.max_iters == 0 and (np.bincount(tries, minlength=4) > 0).all()
        assert np.abs(err - rerr).max() <= 1e-14
        stats_are_sums(st, it, err, 1e-9)


@pytest.mark.parametrize("nj", F.HOME_NJS)
def test_restarts_from_the_home_pose(ctx, nj):
    from inversekinematicsann_amd.kinematics import chain as C
    dh, p = F.table(nj), F.home_fixture(nj)
    R, cap = F.HOME_RESTARTS, F.HOME_ITER[nj]
    a0, i0, t0, e0, s0 = ctx.chain_solve(dh, p, None, None, 1e-6, cap, F.DAMPING, 0)
    ang, it, tries, err, st = ctx.chain_solve(dh, p, None, None, 1e-6, cap, F.DAMPING, R)
    print(f"nj {nj}: capped {s0.n_capped} with no restart, {st.n_capped} with {R} (restatement "
          f"{F.HOME_CAPPED[nj]}); attempts returned {np.bincount(tries, minlength=R + 1)}")
    assert st.n_capped < s0.n_capped and s0.n_capped > 0
    assert not t0.any() and tries.max() <= R and (tries > 0).any()
    stats_are_sums(s0, i0, e0, 1e-6)
    stats_are_sums(st, it, err, 1e-6)
    conv = err <= 1e-6
    assert (round_trip(dh, ang, p)[conv] <= 1e-6 + 1e-12).all() and np.isfinite(ang).all()
    done0 = e0 <= 1e-6  # rows attempt 0 solves are attempt 0's
    assert same(ang[done0], a0[done0]) and same(it[done0], i0[done0]) and not tries[done0].any()
    # the returned attempt alone, from its own start point: the same bits, no more steps
    start = np.tile(dh[0], (len(p), 1))
    for a in range(1, R + 1):
        rows = np.flatnonzero(tries == a)
        u = np.stack([C.start_u(rows, a, j) for j in range(nj)], axis=1)
        start[rows] = -np.pi + u * (np.pi - -np.pi)
    one = ctx.chain_solve(dh, p, start, None, 1e-6, cap, F.DAMPING, 0)
    assert same(one[0], ang) and same(one[3], err)
    assert (it >= one[1]).all() and (it[tries > 0] >= one[1][tries > 0] + cap).all()


# 6 ---------------------------------------------------------------------------
def test_edge_rows(ctx):
    from inversekinematicsann_amd.kinematics.refine import wrap
    dh = F.table(5)
    p, seed, _ = F.chain_fixture(5)
    q, sd = p[:130].copy(), seed[:130] + 7.0
    q[67, 1] = np.nan          # a NaN goal
    q[3] = [50.0, 0.0, 0.0]    # out of reach
    clean = ctx.chain_solve(dh, p[:130], sd, None, 1e-9, 20, F.DAMPING, 2)
    ang, it, tries, err, st = ctx.chain_solve(dh, q, sd, None, 1e-9, 20, F.DAMPING, 2)
    assert it[67] == 0 and tries[67] == 0 and np.isnan(err[67]) and same(ang[67], wrap(sd[67]))
    assert it[3] == 60 and err[3] > 1e-9 and np.isfinite(ang[3]).all()
    assert st.n_capped == 2 and st.first_err == 3 and st.first_err_code == 1
    keep = np.ones(130, bool)
    keep[[3, 67]] = False
    assert all(same(a[keep], b[keep]) for a, b in zip((ang, it, tries, err), clean[:4]))
    stats_are_sums(st, it, err, 1e-9)
    # only NaN rows fail: first_err stays -1
    ang, it, tries, err, st = ctx.chain_solve(dh, q[60:70], sd[60:70], None, 1e-9, 20, F.DAMPING, 2)
    assert (st.n_capped, st.first_err, st.first_err_code) == (1, -1, 0)
    # some |alpha| > 2 pi: every error NaN, no step
    bad = np.array(dh)
    bad[3, 2] = 7.0
    ang, it, tries, err, st = ctx.chain_solve(bad, p[:70], seed[:70], None, 1e-6, 20, F.DAMPING, 2)
    assert not it.any() and not tries.any() and np.isnan(err).all() and same(ang, wrap(seed[:70]))
    assert (st.n_capped, st.first_err, st.max_iters, st.max_fk_err) == (70, -1, 0, 0.0)


# 7 ---------------------------------------------------------------------------
@pytest.mark.parametrize("nj", [3, 5, 8])
def test_device_pointers(ctx, nj):
    import torch
    from inversekinematicsann_amd import _native as N
    dh = F.table(nj)
    p, seed, _ = F.chain_fixture(nj)
    p, seed = p[:321], seed[:321]
    lim = [None] + [(-np.pi / 2, np.pi / 2)] * (nj - 1)
    want = ctx.chain_solve(dh, p, seed, lim, 1e-9, F.MAX_ITER, F.DAMPING, 1)
    dp, ds = torch.from_numpy(p.copy()).cuda(), torch.from_numpy(seed.copy()).cuda()
    # (one buffer, the angles 8 bytes into it: rows of nj doubles need no 16-byte alignment)
    buf = torch.empty(321 * nj + 1, dtype=torch.float64, device="cuda")
    da = buf[1:].view(321, nj)
    assert da.data_ptr() % 16 == 8
    di = torch.empty(321, dtype=torch.int32, device="cuda")
    dt = torch.empty(321, dtype=torch.int32, device="cuda")
    de = torch.empty(321, dtype=torch.float64, device="cuda")
    for flags in (N.IK_F_DEVICE, N.IK_F_DEVICE | N.IK_F_ASYNC | N.IK_F_NO_LIMITS):
        for t in (da, di, dt, de):
            t.zero_()
        st = ctx.chain_solve_device(dh, dp, da, ds, di, dt, de, lim, 1e-9, F.MAX_ITER, F.DAMPING, 1,
                                    flags)
        if flags & N.IK_F_ASYNC:
            st = ctx.stats_fetch()
        got = (da.cpu().numpy(), di.cpu().numpy(), dt.cpu().numpy(), de.cpu().numpy())
        assert all(same(g, w) for g, w in zip(got, want[:4])) and stats_equal(st, want[4], ())
    # no seed array: the table's theta row for every row
    home = ctx.chain_solve(dh, p, None, None, 1e-6, 10, F.DAMPING, 1)
    tiled = ctx.chain_solve(dh, p, np.tile(dh[0], (321, 1)), None, 1e-6, 10, F.DAMPING, 1)
    assert all(same(g, w) for g, w in zip(home[:4], tiled[:4])) and stats_equal(home[4], tiled[4], ())
    ctx.chain_solve_device(dh, dp, da, None, di, dt, de, None, 1e-6, 10, F.DAMPING, 1)
    assert same(da.cpu().numpy(), home[0]) and same(dt.cpu().numpy(), home[2])
    # absent outputs
    only = ctx.chain_solve(dh, p, seed, lim, 1e-9, F.MAX_ITER, F.DAMPING, 1, want_iters=False,
                           want_tries=False, want_fk_err=False)
    assert same(only[0], want[0]) and only[1] is None and stats_equal(only[4], want[4], ())


# 8 ---------------------------------------------------------------------------
def test_abi_refusals(ctx):
    from inversekinematicsann_amd import _native as N
    L, h = ctx.lib, ctx.handle
    inf, nan, pi = np.inf, np.nan, np.pi
    dh = np.ascontiguousarray(F.table(6))
    p, seed, _ = F.chain_fixture(6)
    p, seed = np.ascontiguousarray(p[:8]), np.ascontiguousarray(seed[:8])
    ang, it, tr, err = np.empty((8, 6)), np.empty(8, np.int32), np.empty(8, np.int32), np.empty(8)
    st = N.IkStats()
    ctx.set_joint_limits(LIM)
    held = ctx.joint_limits()

    def call(c=h, nj=6, dh=dh, lo=None, hi=None, pts=p, seed=seed, n=8, tol=1e-6, max_iter=30,
             damping=1e-3, restarts=1, ang=ang, flags=0):
        ptr = lambda a: None if a is None else np.ascontiguousarray(a, np.float64).ctypes.data  # noqa: E731
        keep = [np.ascontiguousarray(a, np.float64) if a is not None else None for a in (lo, hi)]
        return L.ik_chain_solve(c, nj, ptr(dh), ptr(keep[0]), ptr(keep[1]), ptr(pts), ptr(seed), n,
                                tol, max_iter, damping, restarts, ptr(ang) if ang is None else
                                ang.ctypes.data, it.ctypes.data, tr.ctypes.data, err.ctypes.data,
                                flags, ctypes.byref(st))

    def refused(word, **kw):
        assert call(**kw) == N.IK_E_BADARG, kw
        msg = L.ik_last_error().decode()
        assert "ik_chain_solve" in msg and word in msg, msg

    try:
        assert call() == N.IK_OK and (err <= 1e-6).all()
        for nj in (1, 9, 0, -3):
            refused("longer chains are not built", nj=nj)
        refused("dh is NULL", dh=None)
        for r, word in ((1, "non-finite"), (2, "non-finite"), (3, "non-finite")):
            for v in (nan, inf):
                t = dh.copy()
                t[r, 4] = v
                refused("joint 5: a non-finite", dh=t)
        ok_lo, ok_hi = np.full(6, -1.0), np.full(6, 1.0)
        for joint, word, v_lo, v_hi in ((1, "NaN", nan, 1.0), (3, "NaN", 0.0, nan),
                                        (2, "lo > hi", 1.0, 0.5), (6, "outside", -3.2, 1.0),
                                        (4, "outside", 0.0, np.nextafter(pi, 4)),
                                        (5, "infinite", -inf, 1.0), (2, "infinite", 0.0, inf)):
            lo, hi = ok_lo.copy(), ok_hi.copy()
            lo[joint - 1], hi[joint - 1] = v_lo, v_hi
            refused(f"joint {joint}: ", lo=lo, hi=hi)
            assert word in L.ik_last_error().decode()
        refused("both", lo=ok_lo)
        refused("both", hi=ok_hi)
        refused("restarts", restarts=256)
        refused("restarts", restarts=-1)
        refused("max_iter * (restarts + 1)", max_iter=2 ** 31 - 1, restarts=1)
        refused("max_iter * (restarts + 1)", max_iter=2 ** 23, restarts=255)
        assert call(max_iter=2 ** 31 - 1, restarts=0) == N.IK_OK and it.max() < 30
        # what ik_refine refuses
        refused("bad args", n=-1)
        refused("bad args", pts=None)
        refused("bad args", ang=None)
        refused("bad args", max_iter=-1)
        refused("tol is NaN", tol=nan)
        for d in (0.0, -1e-3, nan, inf):
            refused("damping", damping=d)
        refused("IK_F_ASYNC requires IK_F_DEVICE", flags=N.IK_F_ASYNC)
        assert call(c=None) == N.IK_E_BADARG
        # n == 0: IK_OK with empty stats, whatever the arrays
        assert call(n=0, pts=None, seed=None, ang=None) == N.IK_OK
        assert (st.first_oob, st.first_err, st.first_err_code, st.max_iters, st.sum_iters,
                st.n_capped, st.max_fk_err, st.sum_fk_err) == (-1, -1, 0, 0, 0, 0, 0.0, 0.0)
        # a free theta row is a seed, not a refusal; IK_F_NO_LIMITS has no effect
        first = (ang.copy(), it.copy(), tr.copy(), err.copy())
        assert call(flags=N.IK_F_NO_LIMITS) == N.IK_OK
        assert all(same(a, b) for a, b in zip(first, (ang, it, tr, err))) and st.first_oob == -1
        # the next valid call still works, and the context's own limits were not touched
        assert call(lo=ok_lo, hi=ok_hi) == N.IK_OK and np.isfinite(ang).all()
        now = ctx.joint_limits()
        assert same(now[0], held[0]) and same(now[1], held[1])
        with pytest.raises(N.NativeError) as ei:  # the wrapper hands the pair to the library
            ctx.chain_solve(dh, p, seed, None, 1e-6, 30, 0.0)
        assert ei.value.code == N.IK_E_BADARG and "damping" in str(ei.value)
    finally:
        ctx.set_joint_limits(None)


# 9 ---------------------------------------------------------------------------
def test_two_joints_under_limits_through_the_class_and_cli(tmp_path, capsys):
    """At nj = 2 a pair of arrays and two per-joint entries have the same length: the
    class and the command line must hand the library joint 1's and joint 2's own
    intervals, not their transpose."""
    import pandas as pd
    from inversekinematicsann_amd import _native
    from inversekinematicsann_amd.cli import main
    from inversekinematicsann_amd.kinematics.chain import (ChainInverseKinematics,
                                                           chain_refine_reference)
    dh = F.table(2)
    p, seed, th = F.chain_fixture(2)
    p, seed, th = p[:300], seed[:300], th[:300]
    entries = [(-1.25, 1.5), (-0.5, 0.75)]  # asymmetric, and different per joint
    lo, hi = np.array([-1.25, -0.5]), np.array([1.5, 0.75])
    ik = ChainInverseKinematics(dh, entries, tol=1e-9, max_iter=30, restarts=2, strict=False)
    got = np.array(ik.ikine(p.tolist(), seed))
    want = _native.context().chain_solve(dh, p, seed, (lo, hi), 1e-9, 30, 1e-3, 2)
    assert same(got, want[0]) and same(ik.last_fk_err, want[3]) and same(ik.last_tries, want[2])
    assert ((got >= lo) & (got <= hi)).all()
    assert (got[:, 0] == lo[0]).any() and (got[:, 1] == hi[1]).any()  # each joint on its own bound
    inside = ((th >= lo) & (th <= hi)).all(axis=1)
    conv = ik.last_fk_err <= 1e-9
    print(f"{int(inside.sum())} of 300 goals' angles lie inside the limits, {int(conv.sum())} rows "
          f"converged, {int(((got == lo) | (got == hi)).any(axis=1).sum())} end on a limit")
    assert inside.sum() > 50 and conv[inside].all()
    assert (round_trip(dh, got, p)[conv] <= 1e-9 + 1e-12).all()
    rth, rit, rtr, rerr = chain_refine_reference(p, seed, 1e-9, 30, 1e-3, dh, entries, restarts=2)
    # Against the restatement on the rows both call converged: a converged row stops at its
    # first attempt below tol, so its attempt and steps do not hang on rounding (test 2's
    # rule over three attempts).  A goal that cannot be reached inside the limits ends every
    # attempt on the same point of the bound: the attempts' errors tie to the last bits (in
    # the restatement 77 of the 84 rows a later attempt wins, it wins by under 1e-12 of the
    # error), so which of them is returned is rounding's choice and is not compared.
    both = conv & (rerr <= 1e-9)
    eq = (ik.last_iters == rit) & (ik.last_tries == rtr)
    print(f"{int(both.sum())} rows converged in both, {int((~eq[both]).sum())} of them differ in "
          f"steps or attempt; of the others {int((~eq[~both]).sum())} of {int((~both).sum())} do")
    assert both.sum() > 50 and eq[both].mean() >= 0.99
    assert np.array_equal(((got == lo) | (got == hi))[both & eq],
                          ((rth == lo) | (rth == hi))[both & eq])
    assert (ik.last_iters[~both] == 90).all() and (rit[~both] == 90).all()
    # the command line: the same fields, the same angles
    dh_csv, pts_csv, sd_csv, out_csv = (tmp_path / n for n in ("dh.csv", "p.csv", "s.csv", "o.csv"))
    np.savetxt(dh_csv, dh, delimiter=",", fmt="%.17g")
    pd.DataFrame(p, columns=["x", "y", "z"]).to_csv(pts_csv, index=False)
    pd.DataFrame(seed, columns=["theta1", "theta2"]).to_csv(sd_csv, index=False)
    rc = main(["--inverse-kine", "--method", "chain", "--dh", str(dh_csv), "--points", str(pts_csv),
               "--seed-angles", str(sd_csv), "--joint-limits=-1.25:1.5,-0.5:0.75", "--restarts", "2",
               "--tol", "1e-9", "--max-iter", "30", "--to-file", str(out_csv)])
    assert rc == 0
    # (a row above tol: the exception is printed and nothing written, as for the other methods)
    assert "not reached" in capsys.readouterr().out and not out_csv.exists()
    ok = np.flatnonzero(conv)
    pd.DataFrame(p[ok], columns=["x", "y", "z"]).to_csv(pts_csv, index=False)
    pd.DataFrame(seed[ok], columns=["theta1", "theta2"]).to_csv(sd_csv, index=False)
    rc = main(["--inverse-kine", "--method", "chain", "--dh", str(dh_csv), "--points", str(pts_csv),
               "--seed-angles", str(sd_csv), "--joint-limits=-1.25:1.5,-0.5:0.75", "--restarts", "2",
               "--tol", "1e-9", "--max-iter", "30", "--to-file", str(out_csv)])
    assert rc == 0
    csv = pd.read_csv(out_csv, float_precision="round_trip").values
    want = _native.context().chain_solve(dh, pd.read_csv(pts_csv).values, pd.read_csv(sd_csv).values,
                                         (lo, hi), 1e-9, 30, 1e-3, 2)[0]
    assert csv.shape == (len(ok), 2) and np.array_equal(csv, want)
    assert ((csv >= lo) & (csv <= hi)).all()


def test_api_and_cli(tmp_path, capsys):
    import pandas as pd
    from inversekinematicsann_amd import _native
    from inversekinematicsann_amd.cli import main
    from inversekinematicsann_amd.kinematics.chain import ChainInverseKinematics
    from inversekinematicsann_amd.robot.robot import OutOfRobotReachException
    nj = 6
    dh = F.table(nj)
    p = F.home_fixture(nj)[:40]
    jl = [None] + [(-3.0, 3.0)] * (nj - 1)
    ik = ChainInverseKinematics(dh, jl, tol=1e-6, max_iter=30, restarts=4)
    got = ik.ikine(p.tolist())
    want, it, tries, err, st = _native.context().chain_solve(dh, p, None, jl, 1e-6, 30, 1e-3, 4)
    assert got == want.tolist() and isinstance(got[0][0], float) and len(got[0]) == nj
    assert same(ik.last_iters, it) and same(ik.last_tries, tries) and same(ik.last_fk_err, err)
    assert stats_equal(ik.last_stats, st, ()) and st.n_capped == 0
    assert (round_trip(dh, want, p) <= 1e-6 + 1e-12).all()
    seeded = ik.ikine(p.tolist(), seed=want)
    assert seeded == want.tolist() and not ik.last_iters.any()
    # strict: the lowest failing row raises; without, the angles come back
    far = p.copy()
    far[[5, 9]] = [[40.0, 0.0, 0.0], [0.0, 40.0, 0.0]]
    with pytest.raises(OutOfRobotReachException, match=r"point \[40\.0, 0\.0, 0\.0\] not reached"):
        ik.ikine(far.tolist())
    assert ik.last_stats.first_err == 5 and ik.last_stats.n_capped == 2
    loose = ChainInverseKinematics(dh, jl, tol=1e-6, max_iter=30, restarts=4, strict=False)
    out = np.array(loose.ikine(far.tolist()))
    assert np.isfinite(out).all() and loose.last_stats.n_capped == 2
    # the command line writes what the API returns
    dh_csv, pts_csv, out_csv = tmp_path / "dh.csv", tmp_path / "p.csv", tmp_path / "out.csv"
    np.savetxt(dh_csv, dh, delimiter=",", fmt="%.17g")
    pd.DataFrame(p, columns=["x", "y", "z"]).to_csv(pts_csv, index=False)
    rc = main(["--inverse-kine", "--method", "chain", "--dh", str(dh_csv), "--points", str(pts_csv),
               "--joint-limits=" + "," + ",".join(["-3:3"] * (nj - 1)), "--restarts", "4",
               "--refine-tol", "1e-6", "--max-iter", "30", "--to-file", str(out_csv), "--verbose"])
    assert rc == 0
    printed = capsys.readouterr().out
    assert f"chain: {nj} joints, tol 1e-06" in printed and "0 not converged" in printed
    csv = pd.read_csv(out_csv, float_precision="round_trip")
    assert list(csv.columns) == [f"theta{i + 1}" for i in range(nj)]
    # (from the points as the command line reads them: pandas' default parser)
    want = _native.context().chain_solve(dh, pd.read_csv(pts_csv).values, None, jl, 1e-6, 30, 1e-3,
                                         4)[0]
    assert csv.values.dtype == np.float64 and np.array_equal(csv.values, want)
