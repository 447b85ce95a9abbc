"""ik_chain_pose_solve on the GPU: chain_pose_kernel<NJ, kLimited> against ik_chain_solve
bit for bit when the rotation carries no weight, against the numpy restatement
(kinematics/chain.py chain_pose_reference) on the stable rows of
tests/chain_pose_fixtures.py, under limits, with restarts, on edge rows, through device
pointers, its refusals, and the class and command line on top."""
import ctypes

import numpy as np
import pytest

from tests import chain_fixtures as F
from tests import chain_pose_fixtures as PF
from tests.robots import GEN_A, SIXDOF_DH, refine_fixture
from tests.test_gpu_chain import stats_equal
from tests.test_gpu_refine import same
from tests.test_refine_limits_cpu import LIM

pytestmark = pytest.mark.gpu

W = PF.ROT_WEIGHT


@pytest.fixture(scope="module")
def ctx():
    from inversekinematicsann_amd import _native
    c = _native.Context(0)
    yield c
    c.close()


def stats_are_sums(st, it, ep, er, tol, rot_tol):
    n = len(it)
    capped = ~((ep <= tol) & (er <= rot_tol))
    fin = np.isfinite(ep)
    first = np.flatnonzero(capped & fin & np.isfinite(er))
    assert st.first_oob == -1
    assert st.max_iters == (int(it.max()) if n else 0) and st.sum_iters == int(it.sum())
    assert st.n_capped == int(capped.sum())
    assert st.first_err == (int(first[0]) if len(first) else -1)
    assert st.first_err_code == (1 if len(first) else 0)
    assert st.max_fk_err == (ep[fin].max() if fin.any() else 0.0)
    assert abs(st.sum_fk_err - ep[fin].sum()) <= 1e-12 * max(n, 1)


def round_trip(dh, ang, p, G):
    """(|p - FK|, chord) through the long-double product that shares nothing with the
    library."""
    lp, lR = PF.pose_longdouble(dh, ang)
    return (np.linalg.norm((lp - p).astype(np.float64), axis=1),
            PF.chord(lR, G).astype(np.float64))


# 1 ---------------------------------------------------------------------------
@pytest.mark.parametrize("limited", [False, True], ids=["free", "limited"])
@pytest.mark.parametrize("nj", (2, 4, 6, 8))
def test_no_rotation_weight_gives_ik_chain_solve_bits(ctx, nj, limited):
    """Ties the linear half of the new kernel to the old one: a wrong sum order in a
    linear entry of A, a wrong pivot order or a lost lock changes a bit."""
    if nj == 4:
        dh = GEN_A
        p, sd, _ = refine_fixture(GEN_A)
    else:
        dh = F.table(nj)
        p, sd, _ = F.chain_fixture(nj)
    G = np.random.default_rng(nj).normal(size=(len(p), 3, 3))  # any finite G
    lim = [None] + [(-1.0, 1.0)] * (nj - 1) if limited else None
    for seed, cap, restarts in ((sd, 30, 0), (None, 6, 2)):
        want = ctx.chain_solve(dh, p, seed, lim, 1e-9, cap, F.DAMPING, restarts)
        got = ctx.chain_pose_solve(dh, p, G, seed, lim, 1e-9, np.inf, 0.0, cap, F.DAMPING, restarts)
        assert all(same(g, w) for g, w in zip(got[:4], want[:4])), (nj, limited, restarts)
        assert stats_equal(got[5], want[4], ()) and np.isfinite(got[4]).all()
        if restarts:
            assert got[2].any()
        if limited:
            assert ((got[0] == -1.0) | (got[0] == 1.0)).any()
        seed_n = (lambda n: None) if seed is None else (lambda n: seed[:n])
        for n in (0, 1, 63, 64, 65, 257):
            a = ctx.chain_pose_solve(dh, p[:n], G[:n], seed_n(n), lim, 1e-9, np.inf, 0.0, cap,
                                     F.DAMPING, restarts)
            assert a[0].shape == (n, nj) and a[4].shape == (n,)
            assert all(same(g[:n], w) for g, w in zip(got[:5], a[:5]))
            b = ctx.chain_solve(dh, p[:n], seed_n(n), lim, 1e-9, cap, F.DAMPING, restarts)
            assert stats_equal(a[5], b[4], ())


# 2 ---------------------------------------------------------------------------
@pytest.mark.parametrize("tol", PF.TOLS)
@pytest.mark.parametrize("nj", PF.NJS)
def test_parity_with_restatement(ctx, nj, tol):
    """Fails on a wrong axis or frame column, which test 1 cannot see."""
    dh = F.table(nj)
    p, G, seed, _ = PF.pose_fixture(nj)
    ang, it, tries, ep, er, st = ctx.chain_pose_solve(dh, p, G, seed, None, tol, tol, W,
                                                      PF.MAX_ITER[nj], PF.DAMPING, 0)
    rth, rit, _, _, _ = PF.restated(nj, tol)
    s = PF.stable(nj, tol)
    conv = (ep <= tol) & (er <= tol)
    eq = s & (it == rit)
    d = np.abs(ang[eq] - rth[eq]).max()
    tp, tr = round_trip(dh, ang[s], p[s], G[s])
    _, mats, _ = ctx.fk_chain(dh, ang, with_mats=True)
    last = mats[:, -1]
    fp = np.linalg.norm(last[:, :3, 3] - p, axis=1)
    fr = PF.chord(last[:, :3, :3], G)
    print(f"nj {nj} tol {tol:g}: {int((~s).sum())} rows not stable, {int((~conv).sum())} not "
          f"converged; {int((s & ~eq).sum())} stable rows differ in steps; steps max {it.max()}, "
          f"mean {it.mean():.3f}; max |theta_gpu - theta_ref| on equal-count rows = {d:.3g} (bound "
          f"{PF.ANGLE_BOUND[nj]:.3g}); long double round trip: position {tp.max():.3g}, chord "
          f"{tr.max():.3g}; ik_fk_chain round trip: {fp[s].max():.3g}, {fr[s].max():.3g}")
    assert conv[s].all() and not tries.any()
    assert eq[s].mean() >= 0.999 and (np.abs(it - rit)[s] <= 1).all()
    assert d <= PF.ANGLE_BOUND[nj]
    assert (tp <= tol + 1e-12).all() and (tr <= tol + 1e-12).all()
    assert (fp[s] <= tol + 1e-12).all() and (fr[s] <= tol + 1e-12).all()
    stats_are_sums(st, it, ep, er, tol, tol)


# 3 ---------------------------------------------------------------------------
def test_limits_that_bind_at_seven_joints(ctx):
    dh = F.table(7)
    p, G, seed, _ = PF.pose_fixture(7)
    lo, hi = PF.LIMITS7
    cap = PF.MAX_ITER[7]
    free = ctx.chain_pose_solve(dh, p, G, seed, None, 1e-9, 1e-9, W, cap, PF.DAMPING, 0)
    ang, it, tries, ep, er, st = ctx.chain_pose_solve(dh, p, G, seed, (lo, hi), 1e-9, 1e-9, W, cap,
                                                      PF.DAMPING, 0)
    on = (ang == lo) | (ang == hi)
    rth, rit, _, _, _ = PF.restated_limited7()
    s = PF.stable_limited7()
    eq = s & (it == rit)
    d = np.abs(ang[eq] - rth[eq]).max()
    conv = (ep <= 1e-9) & (er <= 1e-9)
    print(f"{int(on.any(axis=1).sum())} rows end on a limit; {int((~conv).sum())} not converged; "
          f"the free solve leaves {int(((free[0] < lo) | (free[0] > hi)).any(axis=1).sum())} rows "
          f"outside; {int((s & ~eq).sum())} stable rows differ in steps; max |theta_gpu - "
          f"theta_ref| = {d:.3g} (bound {PF.LIMITED7_ANGLE_BOUND:.3g})")
    assert ((ang >= lo) & (ang <= hi)).all() and on.any() and not same(ang, free[0])
    assert ((free[0] < lo) | (free[0] > hi)).any()
    assert conv[s].all() and eq[s].mean() >= 0.999 and (np.abs(it - rit)[s] <= 1).all()
    assert d <= PF.LIMITED7_ANGLE_BOUND
    assert np.array_equal(on[eq], ((rth == lo) | (rth == hi))[eq])
    tp, tr = round_trip(dh, ang[s], p[s], G[s])
    assert (tp <= 1e-9 + 1e-12).all() and (tr <= 1e-9 + 1e-12).all()
    stats_are_sums(st, it, ep, er, 1e-9, 1e-9)


# 4 ---------------------------------------------------------------------------
def test_restart_start_points(ctx):
    """No step is taken, so a row's angles are a placed start point: equal bit for bit
    wherever the kernel and the restatement return the same attempt."""
    from inversekinematicsann_amd.kinematics.chain import chain_pose_reference
    for nj, lim, seeded in ((7, [None, (-0.5, 0.25), None, (0.1, 0.1), None, None, (-1.0, 2.0)],
                             True), (6, None, False)):
        dh = F.table(nj)
        p, G, seed, _ = PF.pose_fixture(nj)
        seed = seed if seeded else None
        ang, it, tries, ep, er, st = ctx.chain_pose_solve(dh, p, G, seed, lim, 1e-9, 1e-9, W, 0,
                                                          PF.DAMPING, 3)
        rth, rit, rtr, rep, rer = chain_pose_reference(p, G, seed, 1e-9, 1e-9, W, 0, PF.DAMPING, dh,
                                                       lim, restarts=3)
        agree = tries == rtr
        print(f"nj {nj}: attempts returned {np.bincount(tries, minlength=4)}, "
              f"{int((~agree).sum())} rows differ from the restatement; max |er - er_ref| = "
              f"{np.abs(er - rer).max():.3g}")
        assert agree.mean() >= 0.999 and same(ang[agree], rth[agree])
        assert not it.any() and st.max_iters == 0 and (np.bincount(tries, minlength=4) > 0).all()
        assert np.abs(er - rer).max() <= 1e-14 and np.abs(ep - rep)[agree].max() <= 1e-14
        stats_are_sums(st, it, ep, er, 1e-9, 1e-9)


# 5 ---------------------------------------------------------------------------
def test_restarts_from_the_home_pose(ctx):
    from inversekinematicsann_amd.kinematics import chain as C
    nj, R, cap = PF.HOME_NJ, PF.HOME_RESTARTS, PF.HOME_ITER
    dh = F.table(nj)
    p, G = PF.home_fixture()
    a0, i0, t0, e0, r0, s0 = ctx.chain_pose_solve(dh, p, G, None, None, 1e-6, 1e-6, W, cap,
                                                  PF.DAMPING, 0)
    ang, it, tries, ep, er, st = ctx.chain_pose_solve(dh, p, G, None, None, 1e-6, 1e-6, W, cap,
                                                      PF.DAMPING, R)
    print(f"capped {s0.n_capped} with no restart, {st.n_capped} with {R} (restatement "
          f"{PF.HOME_CAPPED}); attempts returned {np.bincount(tries, minlength=R + 1)}")
    assert st.n_capped < s0.n_capped and s0.n_capped > 0
    assert not t0.any() and tries.max() <= R and (tries > 0).any()
    stats_are_sums(s0, i0, e0, r0, 1e-6, 1e-6)
    stats_are_sums(st, it, ep, er, 1e-6, 1e-6)
    conv = (ep <= 1e-6) & (er <= 1e-6)
    tp, tr = round_trip(dh, ang[conv], p[conv], G[conv])
    assert (tp <= 1e-6 + 1e-12).all() and (tr <= 1e-6 + 1e-12).all() and np.isfinite(ang).all()
    done0 = (e0 <= 1e-6) & (r0 <= 1e-6)  # rows attempt 0 solves are attempt 0's
    assert same(ang[done0], a0[done0]) and same(it[done0], i0[done0]) and not tries[done0].any()
    # the returned attempt alone, from its own start point: the same bits, no more steps
    start = np.tile(dh[0], (len(p), 1))
    for a in range(1, R + 1):
        rows = np.flatnonzero(tries == a)
        u = np.stack([C.start_u(rows, a, j) for j in range(nj)], axis=1)
        start[rows] = -np.pi + u * (np.pi - -np.pi)
    one = ctx.chain_pose_solve(dh, p, G, start, None, 1e-6, 1e-6, W, cap, PF.DAMPING, 0)
    assert same(one[0], ang) and same(one[3], ep) and same(one[4], er)
    assert (it >= one[1]).all() and (it[tries > 0] >= one[1][tries > 0] + cap).all()


# 6 ---------------------------------------------------------------------------
def test_edge_rows(ctx):
    from inversekinematicsann_amd.kinematics.refine import wrap
    nj, tol, cap = 7, 1e-9, 20
    dh = F.table(nj)
    p, G, seed, _ = (a[:130] for a in PF.pose_fixture(nj))
    sd = seed + 2 * np.pi  # (wrapped by the kernel)
    q, H = p.copy(), G.copy()
    q[67, 1] = np.nan                       # a NaN in p
    H[12, 2, 0] = np.nan                    # a NaN in G
    q[3] = [50.0, 0.0, 0.0]                 # an unreachable position
    H[70] = G[70] * np.array([-1.0, -1.0, 1.0])  # reachable, G turned by pi about the tool's z
    H[99] = 2 * G[99]                       # not orthonormal
    edge = [3, 12, 67, 70, 99]
    clean = ctx.chain_pose_solve(dh, p, G, sd, None, tol, tol, W, cap, PF.DAMPING, 2)
    ang, it, tries, ep, er, st = ctx.chain_pose_solve(dh, q, H, sd, None, tol, tol, W, cap,
                                                      PF.DAMPING, 2)
    assert it[67] == 0 and tries[67] == 0 and np.isnan(ep[67]) and same(ang[67], wrap(sd[67]))
    assert it[12] == 0 and tries[12] == 0 and np.isnan(er[12]) and np.isfinite(ep[12])
    assert same(ang[12], wrap(sd[12]))
    assert it[3] == 3 * cap and ep[3] > tol and np.isfinite(ang[3]).all()
    assert it[99] == 3 * cap and er[99] > 1.0 and np.isfinite(ang[99]).all()
    conv = (ep <= tol) & (er <= tol)
    print(f"the row turned by pi: ep {ep[70]:.3g}, er {er[70]:.3g}, attempt {tries[70]}, "
          f"{it[70]} steps, converged {bool(conv[70])}")
    assert np.isfinite(ang[70]).all() and (conv[70] or it[70] == 3 * cap)
    assert not conv[[3, 12, 67, 99]].any() and not (er[conv] > tol).any()
    keep = np.ones(130, bool)
    keep[edge] = False
    assert all(same(a[keep], b[keep]) for a, b in zip((ang, it, tries, ep, er), clean[:5]))
    assert st.first_err == 3 and st.first_err_code == 1
    assert st.n_capped == clean[5].n_capped + 4 + (0 if conv[70] else 1)
    stats_are_sums(st, it, ep, er, tol, tol)
    # only NaN rows fail: first_err stays -1
    ok = conv[60:70].sum()
    *_, st = ctx.chain_pose_solve(dh, q[60:70], H[60:70], sd[60:70], None, tol, tol, W, cap,
                                  PF.DAMPING, 2)
    assert ok == 9 and (st.n_capped, st.first_err, st.first_err_code) == (1, -1, 0)
    # some |alpha| > 2 pi: both errors NaN, no step
    bad = np.array(dh)
    bad[3, 2] = 7.0
    ang, it, tries, ep, er, st = ctx.chain_pose_solve(bad, p[:70], G[:70], seed[:70], None, 1e-6,
                                                      1e-6, W, cap, PF.DAMPING, 2)
    assert not it.any() and not tries.any() and np.isnan(ep).all() and np.isnan(er).all()
    assert same(ang, wrap(seed[:70]))
    assert (st.n_capped, st.first_err, st.max_iters, st.max_fk_err) == (70, -1, 0, 0.0)


# 7 ---------------------------------------------------------------------------
@pytest.mark.parametrize("nj", [3, 8])
def test_device_pointers(ctx, nj):
    import torch
    from inversekinematicsann_amd import _native as N
    dh = F.table(nj)
    p, G, seed, _ = (a[:321] for a in PF.pose_fixture(nj))
    lim = [None] + [(-np.pi / 2, np.pi / 2)] * (nj - 1)
    cap = PF.MAX_ITER[nj]
    want = ctx.chain_pose_solve(dh, p, G, seed, lim, 1e-9, 1e-9, W, cap, PF.DAMPING, 1)
    dp, ds = torch.from_numpy(p.copy()).cuda(), torch.from_numpy(seed.copy()).cuda()
    dg = torch.from_numpy(G.reshape(-1, 9).copy()).cuda()
    # (one buffer, the angles 8 bytes into it: rows of nj doubles need no 16-byte alignment)
    buf = torch.empty(321 * nj + 1, dtype=torch.float64, device="cuda")
    da = buf[1:].view(321, nj)
    assert da.data_ptr() % 16 == 8
    di = torch.empty(321, dtype=torch.int32, device="cuda")
    dt = torch.empty(321, dtype=torch.int32, device="cuda")
    de = torch.empty(321, dtype=torch.float64, device="cuda")
    dr = torch.empty(321, dtype=torch.float64, device="cuda")
    for flags in (N.IK_F_DEVICE, N.IK_F_DEVICE | N.IK_F_ASYNC):
        for t in (da, di, dt, de, dr):
            t.zero_()
        st = ctx.chain_pose_solve_device(dh, dp, dg, da, ds, di, dt, de, dr, lim, 1e-9, 1e-9, W, cap,
                                         PF.DAMPING, 1, flags)
        if flags & N.IK_F_ASYNC:
            st = ctx.stats_fetch()
        got = tuple(t.cpu().numpy() for t in (da, di, dt, de, dr))
        assert all(same(g, w) for g, w in zip(got, want[:5])) and stats_equal(st, want[5], ())
    # no seed array: the table's theta row for every row
    home = ctx.chain_pose_solve(dh, p, G, None, None, 1e-6, 1e-6, W, 10, PF.DAMPING, 1)
    tiled = ctx.chain_pose_solve(dh, p, G, np.tile(dh[0], (321, 1)), None, 1e-6, 1e-6, W, 10,
                                 PF.DAMPING, 1)
    assert all(same(g, w) for g, w in zip(home[:5], tiled[:5])) and stats_equal(home[5], tiled[5], ())
    ctx.chain_pose_solve_device(dh, dp, dg, da, None, di, dt, de, dr, None, 1e-6, 1e-6, W, 10,
                                PF.DAMPING, 1)
    assert same(da.cpu().numpy(), home[0]) and same(dr.cpu().numpy(), home[4])
    # absent outputs, on the host and on the device
    only = ctx.chain_pose_solve(dh, p, G, seed, lim, 1e-9, 1e-9, W, cap, PF.DAMPING, 1,
                                want_iters=False, want_tries=False, want_fk_err=False,
                                want_rot_err=False)
    assert same(only[0], want[0]) and only[1] is only[2] is only[3] is only[4] is None
    assert stats_equal(only[5], want[5], ())
    da.zero_()
    st = ctx.chain_pose_solve_device(dh, dp, dg, da, ds, None, None, None, None, lim, 1e-9, 1e-9, W,
                                     cap, PF.DAMPING, 1)
    assert same(da.cpu().numpy(), want[0]) and stats_equal(st, want[5], ())


# 8 ---------------------------------------------------------------------------
def test_abi_refusals(ctx):
    from inversekinematicsann_amd import _native as N
    L, h = ctx.lib, ctx.handle
    inf, nan = np.inf, np.nan
    dh = np.ascontiguousarray(F.table(6))
    p, G, seed, _ = (np.ascontiguousarray(a[:8]) for a in PF.pose_fixture(6))
    ang, it, tr = np.empty((8, 6)), np.empty(8, np.int32), np.empty(8, np.int32)
    ep, er = np.empty(8), np.empty(8)
    st = N.IkStats()
    ctx.set_robot(SIXDOF_DH)
    ctx.set_joint_limits(LIM)
    held = ctx.joint_limits()
    held_fk = ctx.fk(np.full((1, 4), 0.3))[0]

    def call(c=h, nj=6, dh=dh, lo=None, hi=None, pts=p, rot=G, seed=seed, n=8, tol=1e-6,
             rot_tol=1e-6, rot_weight=1.0, max_iter=60, damping=1e-3, restarts=1, ang=ang, flags=0):
        ptr = lambda a: None if a is None else np.ascontiguousarray(a, np.float64).ctypes.data  # noqa: E731
        keep = [np.ascontiguousarray(a, np.float64) if a is not None else None for a in (lo, hi)]
        return L.ik_chain_pose_solve(c, nj, ptr(dh), ptr(keep[0]), ptr(keep[1]), ptr(pts), ptr(rot),
                                     ptr(seed), n, tol, rot_tol, rot_weight, max_iter, damping,
                                     restarts, None if ang is None else ang.ctypes.data,
                                     it.ctypes.data, tr.ctypes.data, ep.ctypes.data, er.ctypes.data,
                                     flags, ctypes.byref(st))

    def refused(word, **kw):
        assert call(**kw) == N.IK_E_BADARG, kw
        msg = L.ik_last_error().decode()
        assert "ik_chain_pose_solve" in msg and word in msg, msg

    try:
        assert call() == N.IK_OK and (ep <= 1e-6).all() and (er <= 1e-6).all()
        refused("rot is NULL", rot=None)
        refused("rot_tol is NaN", rot_tol=nan)
        for w in (nan, inf, -inf, -1e-300):
            refused("rot_weight", rot_weight=w)
        # what ik_chain_solve refuses, under this call's name
        for nj in (1, 9, 0, -3):
            refused("longer chains are not built", nj=nj)
        refused("dh is NULL", dh=None)
        t = dh.copy()
        t[2, 4] = inf
        refused("joint 5: a non-finite", dh=t)
        ok_lo, ok_hi = np.full(6, -1.0), np.full(6, 1.0)
        for joint, word, v_lo, v_hi in ((1, "NaN", nan, 1.0), (2, "lo > hi", 1.0, 0.5),
                                        (6, "outside", -3.2, 1.0), (5, "infinite", -inf, 1.0)):
            lo, hi = ok_lo.copy(), ok_hi.copy()
            lo[joint - 1], hi[joint - 1] = v_lo, v_hi
            refused(f"joint {joint}: ", lo=lo, hi=hi)
            assert word in L.ik_last_error().decode()
        refused("both", lo=ok_lo)
        refused("both", hi=ok_hi)
        refused("restarts", restarts=256)
        refused("restarts", restarts=-1)
        refused("max_iter * (restarts + 1)", max_iter=2 ** 31 - 1, restarts=1)
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
        assert call(n=0, pts=None, rot=None, seed=None, ang=None) == N.IK_OK
        assert (st.first_oob, st.first_err, st.first_err_code, st.max_iters, st.sum_iters,
                st.n_capped, st.max_fk_err, st.sum_fk_err) == (-1, -1, 0, 0, 0, 0, 0.0, 0.0)
        # rot_tol = +inf and rot_weight = 0 are valid; IK_F_NO_LIMITS has no effect
        assert call(rot_tol=inf, rot_weight=0.0) == N.IK_OK and (ep <= 1e-6).all()
        assert call() == N.IK_OK
        first = (ang.copy(), it.copy(), tr.copy(), ep.copy(), er.copy())
        assert call(flags=N.IK_F_NO_LIMITS) == N.IK_OK
        assert all(same(a, b) for a, b in zip(first, (ang, it, tr, ep, er))) and st.first_oob == -1
        # the next valid call still works; the context's robot and limits were not touched
        assert call(lo=ok_lo, hi=ok_hi) == N.IK_OK and np.isfinite(ang).all()
        now = ctx.joint_limits()
        assert same(now[0], held[0]) and same(now[1], held[1])
        assert same(ctx.fk(np.full((1, 4), 0.3))[0], held_fk)
        with pytest.raises(N.NativeError) as ei:  # the wrapper hands the values to the library
            ctx.chain_pose_solve(dh, p, G, seed, None, 1e-6, 1e-6, 1.0, 30, 0.0)
        assert ei.value.code == N.IK_E_BADARG and "damping" in str(ei.value)
    finally:
        ctx.set_joint_limits(None)
        ctx.set_robot(SIXDOF_DH)


# 9 ---------------------------------------------------------------------------
def test_api_and_cli(ctx, tmp_path, capsys):
    import pandas as pd
    from inversekinematicsann_amd import _native
    from inversekinematicsann_amd.cli import POSE_COLUMNS, main
    from inversekinematicsann_amd.kinematics.chain import ChainInverseKinematics
    from inversekinematicsann_amd.robot.robot import OutOfRobotReachException
    nj = 6
    dh = F.table(nj)
    p, G, seed, th = (a[:40] for a in PF.pose_fixture(nj))
    # poses as the library's own FK reports them: n x 4 x 4, the last cumulative transform
    M = ctx.fk_chain(dh, th, with_mats=True)[1][:, -1]
    ik = ChainInverseKinematics(dh, tol=1e-6, max_iter=60, restarts=2)
    got = ik.ikine_pose(M, seed)
    pair = ik.ikine_pose((M[:, :3, 3], M[:, :3, :3]), seed)
    want, it, tries, ep, er, st = _native.context().chain_pose_solve(
        dh, M[:, :3, 3], M[:, :3, :3], seed, None, 1e-6, 1e-6, 1.0, 60, 1e-3, 2)
    assert got == want.tolist() == pair and isinstance(got[0][0], float) and len(got[0]) == nj
    assert same(ik.last_iters, it) and same(ik.last_tries, tries) and same(ik.last_fk_err, ep)
    assert same(ik.last_rot_err, er) and stats_equal(ik.last_stats, st, ()) and st.n_capped == 0
    tp, tr = round_trip(dh, want, M[:, :3, 3], M[:, :3, :3])
    assert (tp <= 1e-6 + 1e-12).all() and (tr <= 1e-6 + 1e-12).all()
    again = ik.ikine_pose(M, seed=want)
    assert again == want.tolist() and not ik.last_iters.any()
    # rot_tol and rot_weight reach the library
    loose_rot = ChainInverseKinematics(dh, tol=1e-6, max_iter=60, restarts=0, rot_tol=np.inf,
                                       rot_weight=0.0)
    pos = ChainInverseKinematics(dh, tol=1e-6, max_iter=60, restarts=0).ikine(M[:, :3, 3].tolist(),
                                                                              seed)
    assert loose_rot.ikine_pose(M, seed) == pos
    # strict: the lowest failing row raises, naming both errors; without, the angles come back
    far = M.copy()
    far[5, :3, 3] = [40.0, 0.0, 0.0]
    far[9, :3, :3] = far[9, :3, :3] * np.array([-1.0, 1.0, 1.0])  # a reflection: no rotation
    with pytest.raises(OutOfRobotReachException,
                       match=r"pose at \[40\.0, 0\.0, 0\.0\] not reached.*rotation error"):
        ik.ikine_pose(far, seed)
    assert ik.last_stats.first_err == 5 and ik.last_stats.n_capped == 2
    loose = ChainInverseKinematics(dh, tol=1e-6, max_iter=60, restarts=2, strict=False)
    out = np.array(loose.ikine_pose(far, seed))
    assert np.isfinite(out).all() and loose.last_stats.n_capped == 2
    assert loose.last_rot_err[9] > 1e-6
    # the command line writes what the API returns
    dh_csv, poses_csv, sd_csv, out_csv = (tmp_path / n for n in ("dh.csv", "g.csv", "s.csv", "o.csv"))
    np.savetxt(dh_csv, dh, delimiter=",", fmt="%.17g")
    pd.DataFrame(np.concatenate([p, G.reshape(-1, 9)], axis=1), columns=POSE_COLUMNS).to_csv(
        poses_csv, index=False)
    pd.DataFrame(seed, columns=[f"theta{i + 1}" for i in range(nj)]).to_csv(sd_csv, index=False)
    rc = main(["--inverse-kine", "--method", "chain", "--dh", str(dh_csv), "--poses", str(poses_csv),
               "--seed-angles", str(sd_csv), "--restarts", "2", "--tol", "1e-6", "--rot-tol", "1e-7",
               "--rot-weight", "0.5", "--max-iter", "60", "--to-file", str(out_csv), "--verbose"])
    assert rc == 0
    printed = capsys.readouterr().out
    assert f"chain: {nj} joints, tol 1e-06" in printed and "0 not converged" in printed
    assert "rotation error: max" in printed and "rot-tol 1e-07, rot-weight 0.5" in printed
    csv = pd.read_csv(out_csv, float_precision="round_trip")
    assert list(csv.columns) == [f"theta{i + 1}" for i in range(nj)]
    v = pd.read_csv(poses_csv).to_numpy(np.float64)  # (as the command line reads them)
    want = _native.context().chain_pose_solve(dh, v[:, :3], v[:, 3:], pd.read_csv(sd_csv).values,
                                              None, 1e-6, 1e-7, 0.5, 60, 1e-3, 2)
    assert csv.values.dtype == np.float64 and np.array_equal(csv.values, want[0])
    assert (want[4] <= 1e-7).all()
    # usage errors
    with pytest.raises(SystemExit) as ei:
        main(["--inverse-kine", "--method", "chain", "--dh", str(dh_csv), "--poses", str(poses_csv),
              "--points", str(poses_csv)])
    assert ei.value.code == 2 and "--points or --poses, not both" in capsys.readouterr().err
    with pytest.raises(SystemExit) as ei:
        main(["--inverse-kine", "--method", "chain", "--dh", str(dh_csv), "--points", str(poses_csv),
              "--rot-weight", "2"])
    assert ei.value.code == 2 and "--rot-weight is only valid with --poses" in capsys.readouterr().err
