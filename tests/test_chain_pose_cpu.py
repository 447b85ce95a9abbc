"""ik_chain_pose_solve without a GPU: the ABI's declaration against the binding, the row
header (csrc/ik_chain_pose_row.h) in a stand-alone host program against the numpy
restatement (kinematics/chain.py) byte for byte and against what the chain has to be,
the two rotation errors against their closed forms, the stop rule at a turn of pi, the
restatement with no rotation weight against the position solve's, the stable rows and
measured bounds of tests/chain_pose_fixtures.py, the restart fixture, the kernels'
registers, and the refusals of the Python entry points and of the command line.
tests/test_gpu_chain_pose.py runs the same fixtures through the kernel."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import chain_fixtures as F
from tests import chain_pose_fixtures as PF
from tests.conftest import ROOT
from tests.robots import GEN_A

CLANGXX = "/opt/rocm/llvm/bin/clang++"  # csrc/Makefile HOSTCXX
HIPCC = "/opt/rocm/bin/hipcc"  # csrc/Makefile HIPCC
CSRC = os.path.join(ROOT, "inversekinematicsann_amd", "csrc")
SPECIAL = (0.0, np.pi, -np.pi, np.pi / 2, -np.pi / 2)
EPS = 2.0 ** -53


def same(a, b):
    return a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


def rot_axis(axis, phi):
    """Rodrigues: n x 3 x 3 rotations by phi (n) about the unit vectors axis (n x 3), in
    long double."""
    axis, phi = np.asarray(axis, np.longdouble), np.asarray(phi, np.longdouble)
    K = np.zeros((len(axis), 3, 3), np.longdouble)
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 2] = -axis[:, 2], axis[:, 1], -axis[:, 0]
    K = K - K.transpose(0, 2, 1)
    s, c = np.sin(phi)[:, None, None], np.cos(phi)[:, None, None]
    return np.identity(3, np.longdouble) + s * K + (1 - c) * (K @ K)


# 1 ---------------------------------------------------------------------------
def test_declaration_and_binding_agree():
    import ctypes
    from inversekinematicsann_amd import _native
    hdr = open(os.path.join(ROOT, "include", "ikhip.h")).read()
    m = re.search(r"^int ik_chain_pose_solve\(ik_ctx \*ctx,(.*?)\);", hdr, re.M | re.S)
    assert m and "ik_chain_pose_solve" in _native.EXPORTED_SYMBOLS
    params = [p.strip() for p in
              ("ik_ctx *ctx," + re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)).split(",")]
    kind = {"ik_ctx *": ctypes.c_void_p, "const double *": ctypes.c_void_p,
            "double *": ctypes.c_void_p, "int32_t *": ctypes.c_void_p, "int64_t ": ctypes.c_int64,
            "int32_t ": ctypes.c_int32, "double ": ctypes.c_double, "int ": ctypes.c_int,
            "ik_stats *": ctypes.POINTER(_native.IkStats)}
    names = [re.match(r"(.*?)(\w+)$", p).group(2) for p in params]
    want = [kind[re.match(r"(.*?)(\w+)$", p).group(1)] for p in params]
    assert names == ["ctx", "nj", "dh", "lo", "hi", "pts", "rot", "seed", "n", "tol", "rot_tol",
                     "rot_weight", "max_iter", "damping", "restarts", "ang", "iters", "tries",
                     "fk_err", "rot_err", "flags", "stats"]
    got = _native.load_library().ik_chain_pose_solve.argtypes
    assert len(got) == 22 and list(got) == want


# 2 ---------------------------------------------------------------------------
def _angle_rows(nj, rng, n):
    th = rng.uniform(-np.pi, np.pi, (n, nj))
    sp = np.array([[v] * nj for v in SPECIAL])
    return np.concatenate([th, sp])


def _host_blocks():
    """Per nj = 2..8 a block under limits that bind, a block with every joint free and a
    limited block without rotation weight: (the doubles the program reads, the doubles
    it has to write)."""
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
        rng = np.random.default_rng(70 + nj)
        for limited_block, w in ((True, 0.75), (False, 1.0), (True, 0.0)):
            w = np.float64(w)
            lo, hi = np.full(8, -np.inf), np.full(8, np.inf)
            if limited_block:  # joint 1 free, joint 2 fixed, the others narrow
                lo[1:nj], hi[1:nj] = -0.6, 0.4
                lo[1] = hi[1] = 0.25
            limited = ~(np.isneginf(lo[:nj]) & np.isposinf(hi[:nj]))
            mask = int((limited << np.arange(nj)).sum())
            th = C._place(_angle_rows(nj, rng, 150), lo[:nj], hi[:nj], limited, np.float64)
            gp, gR = C.chain_fk_pose(dh, th + rng.normal(0, 0.3, th.shape))
            gp = gp + rng.normal(0, 0.01, gp.shape)
            G = gR.reshape(-1, 9) + rng.normal(0, 0.01, (len(th), 9))  # (used as given)
            s, c = np.sin(th), np.cos(th)
            (x, y, z), J = C._chain_cs(consts, s, c)
            r, W = C._pose_frame_cs(consts, s, c)
            ew = C._rot_step_error(r, G)
            er = C._rot_error(r, G)
            e = [gp[:, 0] - x, gp[:, 1] - y, gp[:, 2] - z] + [w * v for v in ew]
            if limited_block:
                dl, lock, rs = C._pose_limited_step(J, W, e, w, lam2, th, lo[:nj], hi[:nj], limited)
                assert lock.any() and (nj == 2 or (rs >= 2).any())  # (nj 2: one limited joint)
                if w == 0:
                    d0, lock0, rs0 = C._limited_step(J, e[:3], lam2, th, lo[:nj], hi[:nj], limited)
                    assert all(same(u, v) for u, v in zip(dl, d0)) and same(lock, lock0)
            else:
                dl = C._pose_solve(J, W, e, w, lam2, None)
                lock, rs = np.zeros((len(th), nj), bool), np.zeros(len(th))
            new = C._update(th, dl, lo[:nj], hi[:nj], limited, np.float64)
            cols = [x, y, z] + [r[k][i] for i in range(3) for k in range(3)]
            cols += [col[k] for k in range(3) for col in J] + [ax[k] for k in range(3) for ax in W]
            cols += list(ew) + [er] + list(dl)
            cols += [(lock << np.arange(nj)).sum(axis=1).astype(np.float64), rs.astype(np.float64)]
            want.append(np.concatenate([np.stack(cols, axis=1), new], axis=1).ravel())
            blocks += [np.array([nj, len(th)], np.float64), np.asarray(dh, np.float64).ravel(),
                       jc.ravel(), lo, hi, np.array([mask, lam2, w]),
                       np.concatenate([th, s, c, gp, G], axis=1).ravel()]
    data = np.concatenate([np.array([21.0])] + blocks)
    return data, np.concatenate(want)


@pytest.mark.skipif(not os.path.exists(CLANGXX), reason="the ROCm clang++ is not installed")
def test_row_header_in_host_program(tmp_path):
    """p, R, the six Jacobian rows, e_w, er, delta, the lock mask, the re-solves and
    theta' byte for byte; inside the program: R and p within 50 roundings of the long
    double DH product, axis i = z_{i-1}, linear column i = z_{i-1} x (p - o_{i-1}), the
    position and linear columns chain_jac's bits, and w = 0 chain_step's delta."""
    exe = os.path.join(str(tmp_path), "chain_pose_row_check")
    subprocess.run([CLANGXX, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
                    "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", CSRC,
                    os.path.join(ROOT, "tests", "host", "chain_pose_row_check.cpp"), "-o", exe],
                   check=True)
    data, want = _host_blocks()
    rows, out = tmp_path / "rows.f64", tmp_path / "out.f64"
    data.astype("<f8").tofile(rows)
    r = subprocess.run([exe, str(rows), str(out)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-4000:]
    assert "chain_pose_row_check ok" in r.stdout, r.stdout[-4000:]
    got = np.fromfile(out, "<f8")
    assert got.shape == want.shape
    differ = np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))
    assert got.tobytes() == want.astype("<f8").tobytes(), (differ[:10], got[differ[:5]],
                                                          want[differ[:5]])


# 3 ---------------------------------------------------------------------------
@pytest.mark.parametrize("nj", (2, 3, 4, 5, 6, 7, 8))
def test_pose_against_the_long_double_product(nj):
    """The restatement's p within 50 roundings of the chain's length, its R within 50
    roundings of 1, of the long-double DH product; p is chain_fk's bits."""
    from inversekinematicsann_amd.kinematics.chain import chain_fk, chain_fk_pose
    dh = GEN_A if nj == 4 else F.table(nj)
    th = np.random.default_rng(80 + nj).uniform(-np.pi, np.pi, (256, nj))
    L = np.abs(dh[1]).sum() + np.abs(dh[2]).sum()
    p, R = chain_fk_pose(dh, th)
    lp, lR = PF.pose_longdouble(dh, th)
    dp, dR = np.abs((p - lp).astype(np.float64)).max(), np.abs((R - lR).astype(np.float64)).max()
    print(f"nj {nj}: max |p - long double| = {dp:.3g}, max |R - long double| = {dR:.3g}")
    assert R.shape == (256, 3, 3) and same(p, chain_fk(dh, th))
    assert dp <= 50 * EPS * L and dR <= 50 * EPS


# 4 ---------------------------------------------------------------------------
def test_rotation_errors_against_their_closed_forms():
    """G = R Rot(axis, phi), the axis in the tool frame: er = 2 sin(phi / 2) and e_w =
    sin(phi) R axis.  R and G are rounded from long double (9 entries, half a rounding
    each) and each error is a sum of at most 9 products of entries <= 1: 20 roundings of
    the largest value, 2."""
    from inversekinematicsann_amd.kinematics import chain as C
    dh = F.table(6)
    rng = np.random.default_rng(90)
    n = 512
    th = rng.uniform(-np.pi, np.pi, (n, 6))
    axis = rng.normal(size=(n, 3))
    axis /= np.linalg.norm(axis, axis=1)[:, None]
    phi = np.concatenate([rng.uniform(-np.pi, np.pi, n - 4), [0.0, np.pi, 1e-9, np.pi - 1e-7]])
    _, lR = PF.pose_longdouble(dh, th)
    G = (lR @ rot_axis(axis, phi)).astype(np.float64).reshape(n, 9)
    consts = C._consts(dh, np.float64)
    r, _ = C._pose_frame_cs(consts, np.sin(th), np.cos(th))
    er = C._rot_error(r, G)
    ew = np.stack(C._rot_step_error(r, G), axis=1)
    want_er = (2 * np.abs(np.sin(np.asarray(phi, np.longdouble) / 2))).astype(np.float64)
    want_ew = (np.sin(np.asarray(phi, np.longdouble))[:, None]
               * np.einsum("nij,nj->ni", lR, axis.astype(np.longdouble))).astype(np.float64)
    d_er, d_ew = np.abs(er - want_er).max(), np.abs(ew - want_ew).max()
    print(f"max |er - 2 sin(phi / 2)| = {d_er:.3g}, max |e_w - sin(phi) axis| = {d_ew:.3g}")
    # (the bound is on er^2, the sum; the square root divides it by er + want, and one
    # more rounding of er is the root's own)
    assert (np.abs(er * er - want_er * want_er) <= 20 * EPS * 4).all()
    big = want_er > 1e-3
    assert (np.abs(er - want_er)[big] <= 20 * EPS * 4 / (2 * want_er[big]) + 2 * EPS).all()
    assert d_ew <= 20 * EPS * 2
    assert er[n - 3] == pytest.approx(2.0, abs=40 * EPS) and np.abs(ew[n - 3]).max() <= 40 * EPS


# 5 ---------------------------------------------------------------------------
@pytest.mark.parametrize("nj", (6, 7))
def test_no_false_convergence_at_a_turn_of_pi(nj):
    """The goal is the seed's own pose turned by pi about the tool's z: the position error
    and the step's rotation error vanish, the chord is 2.  A stop rule on |e_w| would
    call every row converged."""
    from inversekinematicsann_amd.kinematics import chain as C
    dh = F.table(nj)
    seed = PF.pose_fixture(nj)[2][:64]
    p, R = C.chain_fk_pose(dh, seed)
    G = R * np.array([-1.0, -1.0, 1.0])  # columns 1 and 2 negated: R Rz(pi)
    consts = C._consts(dh, np.float64)
    r, _ = C._pose_frame_cs(consts, np.sin(C.wrap(seed)), np.cos(C.wrap(seed)))
    ew = np.stack(C._rot_step_error(r, G.reshape(-1, 9)), axis=1)
    assert np.abs(ew).max() <= 50 * EPS
    th, it, tries, ep, er = C.chain_pose_reference(p, G, seed, 1e-6, 1e-6, 1.0, 30, F.DAMPING, dh)
    conv = (ep <= 1e-6) & (er <= 1e-6)
    print(f"nj {nj}: {int(conv.sum())} of 64 converged, er in [{er.min():.17g}, {er.max():.17g}], "
          f"steps max {it.max()}")
    assert not conv.any() and (it == 30).all() and not tries.any()
    assert np.abs(er - 2.0).max() <= 50 * EPS * 2


# 6 ---------------------------------------------------------------------------
@pytest.mark.parametrize("nj", (2, 3, 4, 6, 8))
def test_no_rotation_weight_is_the_position_solve(nj):
    """chain_pose_reference(rot_weight=0, rot_tol=inf) = chain_refine_reference bit for
    bit: free, under limits that bind, and with restarts."""
    from inversekinematicsann_amd.kinematics.chain import (chain_pose_reference,
                                                           chain_refine_reference)
    if nj == 4:
        from tests.robots import refine_fixture
        dh = GEN_A
        p, sd, _ = refine_fixture(GEN_A)
    else:
        dh = F.table(nj)
        p, sd, _ = F.chain_fixture(nj)
    p, sd = p[:700], sd[:700]
    G = np.random.default_rng(nj).normal(size=(len(p), 3, 3))  # any finite G
    lim = [None] + [(-1.0, 1.0)] * (nj - 1)  # (inside the interval theta* was drawn from)
    for jl, seed, cap, restarts in ((None, sd, 30, 0), (lim, sd, 30, 0), (None, None, 6, 2),
                                    (lim, None, 6, 2)):
        want = chain_refine_reference(p, seed, 1e-9, cap, F.DAMPING, dh, jl, restarts=restarts)
        got = chain_pose_reference(p, G, seed, 1e-9, np.inf, 0.0, cap, F.DAMPING, dh, jl,
                                   restarts=restarts)
        assert all(same(g, w) for g, w in zip(got[:4], want)), (nj, jl is None, restarts)
        assert np.isfinite(got[4]).all()
        if restarts:
            assert got[2].any()
        if jl is not None:
            assert ((got[0] == -1.0) | (got[0] == 1.0)).any()


# 7 ---------------------------------------------------------------------------
@pytest.mark.parametrize("nj", PF.NJS)
def test_stable_rows_and_float64_against_long_double(nj):
    dh = F.table(nj)
    p, G, _, _ = PF.pose_fixture(nj)
    for k, tol in enumerate(PF.TOLS):
        t64, i64, tr, ep, er = PF.restated(nj, tol)
        tld, ild, _, _, _ = PF.restated(nj, tol, np.longdouble)
        st = PF.stable(nj, tol)
        d = np.abs(t64[st] - tld[st].astype(np.float64)).max()
        print(f"nj {nj} tol {tol:g}: {int((~st).sum())} of {len(st)} rows not stable "
              f"({int((~((ep <= tol) & (er <= tol))).sum())} not converged in float64, "
              f"{int((i64 != ild).sum())} differ in steps); steps max {i64.max()}, mean "
              f"{i64.mean():.3f}; max |dtheta| = {d:.3g} (written "
              f"{PF.MEASURED_F64_VS_LONGDOUBLE[nj][k]:.3g})")
        assert st.mean() >= PF.STABLE_SHARE
        assert d <= PF.MEASURED_F64_VS_LONGDOUBLE[nj][k]
        assert not tr.any() and np.abs(t64).max() <= np.pi
        # the converged rows by a product that shares nothing with the restatement
        lp, lR = PF.pose_longdouble(dh, t64[st])
        assert (np.linalg.norm((lp - p[st]).astype(np.float64), axis=1) <= tol + 1e-12).all()
        assert (PF.chord(lR, G[st]).astype(np.float64) <= tol + 1e-12).all()
    assert PF.ANGLE_BOUND[nj] == 10 * max(PF.MEASURED_F64_VS_LONGDOUBLE[nj])


def test_limited_restatement_float64_against_long_double():
    lo, hi = PF.LIMITS7
    t64, i64, _, ep, er = PF.restated_limited7()
    tld = PF.restated_limited7(np.longdouble)[0]
    st = PF.stable_limited7()
    d = np.abs(t64[st] - tld[st].astype(np.float64)).max()
    on = (t64 == lo) | (t64 == hi)
    free = PF.restated(7, 1e-9)[0]
    print(f"{int((~st).sum())} rows not stable; max |dtheta| = {d:.3g}; "
          f"{int(on.any(axis=1).sum())} rows end on a limit")
    assert st.mean() >= PF.STABLE_SHARE and ((t64 >= lo) & (t64 <= hi)).all() and on[st].any()
    assert not same(t64, free) and ((free < lo) | (free > hi)).any()
    assert d <= PF.MEASURED_LIMITED7_F64_VS_LONGDOUBLE
    assert PF.LIMITED7_ANGLE_BOUND == 10 * PF.MEASURED_LIMITED7_F64_VS_LONGDOUBLE


# 8 ---------------------------------------------------------------------------
def test_restarts_reduce_capped():
    p, G = PF.home_fixture()
    th0, it0, tr0, ep0, er0 = PF.home_restated(0)
    th, it, tr, ep, er = PF.home_restated(PF.HOME_RESTARTS)
    done0, done = (ep0 <= 1e-6) & (er0 <= 1e-6), (ep <= 1e-6) & (er <= 1e-6)
    capped = (int((~done0).sum()), int((~done).sum()))
    print(f"capped {capped}, attempts returned {np.bincount(tr)}")
    assert capped == PF.HOME_CAPPED and capped[1] < capped[0]
    assert not tr0.any() and tr.max() <= PF.HOME_RESTARTS
    # a row attempt 0 solves is attempt 0's; the others ran every attempt they needed
    assert same(th[done0], th0[done0]) and not tr[done0].any() and same(it[done0], it0[done0])
    assert (it[~done0] > it0[~done0]).all()
    assert (ep + PF.ROT_WEIGHT * er <= ep0 + PF.ROT_WEIGHT * er0).all()


def test_edge_rows_of_the_restatement():
    from inversekinematicsann_amd.kinematics import chain as C
    dh = F.table(6)
    p, G, sd, _ = (a[:6] for a in PF.pose_fixture(6))
    clean = C.chain_pose_reference(p, G, sd, 1e-9, 1e-9, 1.0, 30, 1e-3, dh, restarts=2)
    q, H = p.copy(), G.copy()
    q[1, 0] = np.nan       # a NaN in p: no step, no restart
    H[2, 1, 1] = np.nan    # a NaN in G: the same
    H[4] = 2 * G[4]        # not orthonormal: never converges, finite angles
    th, it, tr, ep, er = C.chain_pose_reference(q, H, sd, 1e-9, 1e-9, 1.0, 30, 1e-3, dh, restarts=2)
    assert it[1] == 0 and tr[1] == 0 and np.isnan(ep[1]) and same(th[1], C.wrap(sd[1]))
    assert it[2] == 0 and tr[2] == 0 and np.isnan(er[2]) and np.isfinite(ep[2])
    assert it[4] == 90 and er[4] > 1.0 and np.isfinite(th[4]).all()
    keep = [0, 3, 5]
    assert all(same(a[keep], b[keep]) for a, b in zip((th, it, tr, ep, er), clean))
    bad = np.array(dh)
    bad[3, 2] = 7.0        # some |alpha| > 2 pi: both errors NaN, no step
    th, it, tr, ep, er = C.chain_pose_reference(p, G, sd, 1e-6, 1e-6, 1.0, 10, 1e-3, bad, restarts=2)
    assert not it.any() and not tr.any() and np.isnan(ep).all() and np.isnan(er).all()
    assert same(th, C.wrap(sd))


# 9 ---------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="the ROCm hipcc is not installed")
def test_no_pose_kernel_uses_scratch(tmp_path):
    """The 6 x NJ matrix and the 6 x 6 factor fill the register file (one wave per SIMD
    from NJ = 6, AGPRs as overflow): what the compiler reports for each of the 14
    instantiations, built with the Makefile's flags, has no scratch and no spilled VGPR."""
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                        "-ffp-contract=off", "-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(CSRC, "ik_chain_pose.hip"), "-o",
                        str(tmp_path / "ik_chain_pose.o")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    names = re.findall(r"Function Name: \w*chain_pose_kernelILi(\d)ELb([01])E", r.stdout)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stdout)]
    spilled = [int(v) for v in re.findall(r"VGPRs Spill: (\d+)", r.stdout)]
    assert sorted(names) == sorted((str(nj), b) for nj in range(2, 9) for b in "01"), names
    assert len(scratch) == len(spilled) == 14
    assert not any(scratch) and not any(spilled), (names, scratch, spilled)


# 10 --------------------------------------------------------------------------
def test_python_entry_points_refuse_without_a_gpu(monkeypatch):
    """The refusals come before the library is loaded or a context made."""
    from inversekinematicsann_amd import _native
    from inversekinematicsann_amd.kinematics.chain import (ChainInverseKinematics, as_poses,
                                                           chain_pose_reference)

    def no_library(*a, **k):
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_native, "load_library", no_library)
    monkeypatch.setattr(_native, "context", no_library)
    ctx = object.__new__(_native.Context)  # (no ik_ctx_create)
    ctx.handle = None
    pts, rot = np.zeros((3, 3)), np.tile(np.eye(3), (3, 1, 1))
    dh6 = F.table(6)
    for kw, word in (({"dh": np.ones((4, 1))}, "not built"), ({"dh": np.ones((4, 9))}, "not built"),
                     ({"joint_limits": (np.zeros(6), None)}, "both"),
                     ({"restarts": 256}, "restarts"), ({"max_iter": -1}, "max_iter"),
                     ({"max_iter": 2 ** 31 - 1, "restarts": 1}, r"max_iter \* \(restarts \+ 1\)"),
                     ({"rot_tol": np.nan}, "rot_tol"), ({"rot_weight": np.nan}, "rot_weight"),
                     ({"rot_weight": -1.0}, "rot_weight"), ({"rot_weight": np.inf}, "rot_weight")):
        args = {"dh": dh6, "pts": pts, "rot": rot, **kw}
        with pytest.raises(ValueError, match=word):
            ctx.chain_pose_solve(**args)
        with pytest.raises(ValueError, match=word):
            ctx.chain_pose_solve_device(ang=None, **args)
        with pytest.raises(ValueError, match=word):
            chain_pose_reference(seed=None, **args)
    for kw, word in (({"rot_tol": np.nan}, "rot_tol"), ({"rot_weight": -0.5}, "rot_weight"),
                     ({"rot_weight": np.inf}, "rot_weight")):
        with pytest.raises(ValueError, match=word):
            ChainInverseKinematics(dh6, **kw)
    ik = ChainInverseKinematics(dh6, tol=1e-7)
    assert ik.rot_tol == 1e-7 and ik.rot_weight == 1.0 and ik.last_rot_err is None
    assert ChainInverseKinematics(dh6, rot_tol=np.inf, rot_weight=0).rot_tol == np.inf
    assert ik.ikine_pose([]) == [] and ik.ikine_pose((np.zeros((0, 3)), np.zeros((0, 3, 3)))) == []
    # both spellings of the poses give the same arrays
    M = np.tile(np.eye(4), (5, 1, 1))
    M[:, :3, :] = np.random.default_rng(1).normal(size=(5, 3, 4))
    a, b = as_poses(M), as_poses((M[:, :3, 3], M[:, :3, :3]))
    assert same(a[0], b[0]) and same(a[1], b[1]) and a[1].shape == (5, 9)
    assert same(a[1][2], M[2, :3, :3].ravel())
    for bad in (np.zeros((5, 3, 3)), np.zeros((4, 4)), (np.zeros((5, 3)), np.zeros((4, 3, 3)))):
        with pytest.raises(ValueError, match="poses"):
            ik.ikine_pose(bad)


def cli_error(argv, capsys):
    from inversekinematicsann_amd.cli import main
    with pytest.raises(SystemExit) as ei:
        main(argv)
    assert ei.value.code == 2
    return capsys.readouterr().err


def test_cli_usage_errors(tmp_path, capsys):
    from inversekinematicsann_amd.cli import POSE_COLUMNS
    assert POSE_COLUMNS == "x,y,z,r11,r12,r13,r21,r22,r23,r31,r32,r33".split(",")
    pts = tmp_path / "p.csv"
    pts.write_text("x,y,z\n1.0,0.5,0.2\n")
    poses = tmp_path / "poses.csv"
    poses.write_text(",".join(POSE_COLUMNS) + "\n1.0,0.5,0.2,1,0,0,0,1,0,0,0,1\n")
    dh = tmp_path / "dh.csv"
    np.savetxt(dh, F.table(6), delimiter=",")
    chain = ["--inverse-kine", "--method", "chain", "--dh", str(dh)]
    assert "required: --points" in cli_error(chain, capsys)
    assert "--points or --poses, not both" in \
        cli_error(chain + ["--points", str(pts), "--poses", str(poses)], capsys)
    assert "--rot-tol is only valid with --poses" in \
        cli_error(chain + ["--points", str(pts), "--rot-tol", "1e-6"], capsys)
    assert "--rot-weight is only valid with --poses" in \
        cli_error(chain + ["--points", str(pts), "--rot-weight", "2"], capsys)
    assert "--rot-weight takes a finite number >= 0" in \
        cli_error(chain + ["--poses", str(poses), "--rot-weight=-1"], capsys)
    assert "--rot-tol takes a number" in \
        cli_error(chain + ["--poses", str(poses), "--rot-tol", "nan"], capsys)
    assert "--poses: the header must be x,y,z,r11" in \
        cli_error(chain + ["--poses", str(pts)], capsys)
    assert "required: --dh" in \
        cli_error(["--inverse-kine", "--method", "chain", "--poses", str(poses)], capsys)
    for flag, val in (("--poses", str(poses)), ("--rot-tol", "1e-6"), ("--rot-weight", "1")):
        assert f"{flag} is only valid with --method chain" in \
            cli_error(["--inverse-kine", "--method", "fabrik", "--points", str(pts), flag, val],
                      capsys)
    assert "required: --points" in \
        cli_error(["--inverse-kine", "--method", "fabrik", "--poses", str(poses)], capsys)
