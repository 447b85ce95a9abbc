"""What tests/test_gpu_robots.py rests on, without a GPU: the oracle's dh= path
pinned to the reference on tables with no zero entry, every table entry shown
to move what the GPU tests bound, the refine restatement on those tables, and
the FABRIK solve's indifference to the last bits of its seed."""
import math
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests import robots as RB
from tests.conftest import GOLDEN

NAMES = list(RB.TABLES)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "robots_general_dh.npz"), allow_pickle=False)


# ------------------------------------------------- oracle against golden ----
@pytest.mark.parametrize("name", NAMES)
def test_oracle_fabrik_dh_path_bit_exact(golden, name):
    dh = RB.TABLES[name]
    assert np.array_equal(golden[f"{name}_dh"], dh)
    assert [(float(t), int(m)) for t, m in zip(golden["tols"], golden["max_iters"])] == \
        list(RB.CONFIGS)
    pts = golden[f"{name}_points"]
    assert O.check_limits(pts, RB.DEFAULT_LIMITS) == -1  # the reference solved every row
    for k, (tol, mi) in enumerate(RB.CONFIGS):
        ang, it, jo, st = O.fabrik_ikine(pts, tol, mi, dh=dh, links=RB.LINKS)
        assert np.array_equal(st, golden[f"{name}_status_{k}"])
        ok = st == 0
        assert np.array_equal(it[ok], golden[f"{name}_iters_{k}"][ok])
        assert np.array_equal(ang[ok], golden[f"{name}_angles_{k}"][ok])  # bit for bit
        assert np.array_equal(jo[ok], golden[f"{name}_joints_{k}"][ok])
        assert 0 < (it[ok] >= mi).sum() < ok.sum()  # capped and converged rows both


@pytest.mark.parametrize("name", NAMES)
def test_oracle_fk_dh_path_against_golden_mats(golden, name):
    dh = RB.TABLES[name]
    ang, mats = golden[f"{name}_fk_angles"], golden[f"{name}_fk_mats"]
    assert mats.shape == (len(ang), 4, 4, 4)
    xyz, jo, st = O.fk(ang, dh)
    assert not st.any()
    assert np.array_equal(jo, mats[:, :, :3, 3])  # all four joints, bit for bit
    assert np.array_equal(xyz, mats[:, 3, :3, 3])
    worst = max(np.abs(np.array(O.fk_n(dh, a)) - m).max() for a, m in zip(ang, mats))
    print(f"{name}: max |fk_n - fkine| over the four matrices = {worst:.3g}")
    assert worst <= 1e-12


# ------------------------------------------------ every constant is live ----
def _seed_joints(dh, pts):
    """The FABRIK seed pose of every goal (inverse.py:123-130)."""
    th = np.tile(np.asarray(dh)[0], (len(pts), 1))
    th[:, 0] = np.arctan2(pts[:, 1], pts[:, 0])
    return O.fk(th, dh)[1]


@pytest.mark.parametrize("name", ["GEN_A", "GEN_B"])
def test_every_constant_is_live(golden, name):
    """Each of the 15 entries the device reads, set to SixDOFRobot's value, moves
    the quantity a GPU test bounds by at least 1e6 x that bound at some row:
      d, a, alpha_1..3  the effector of O.fk (bound 1e-12 on the round trips);
      alpha_4           Rx(alpha_4) is the chain's last factor and moves no
                        position, only the rotation part of the fourth matrix
                        (bound 1e-12 on ctx.fk's mats);
      theta_2..4        the FABRIK seed joints, which a solve of no iteration
                        returns, and the solved angles with them (bound 1e-9 on
                        angles and joints); theta_4 moves the seed's effector
                        alone, which the first backward pass replaces by the goal
                        (fabrik.py:20-22), so it shows only where no pass runs;
      a_1, d_2..4, a_2..4, alpha_1..3
                        also a column of refine's Jacobian (the angles' bound
                        ANGLE_BOUND ~ 1e-12); d_1, alpha_4 and the thetas do not
                        enter it."""
    from inversekinematicsann_amd.kinematics.refine import jacobian
    dh = RB.TABLES[name]
    _, _, th = RB.refine_fixture(dh)
    fk_ang = golden[f"{name}_fk_angles"]
    pts = golden[f"{name}_points"]
    base_xyz = O.fk(th, dh)[0]
    base_J = jacobian(dh, th)
    base_mats = np.array([O.fk_n(dh, a) for a in fk_ang])
    base_seed = _seed_joints(dh, pts)
    base_ang = {mi: O.fabrik_ikine(pts, 1e-3, mi, dh=dh)[0] for mi in (0, 100)}
    in_jacobian = {(1, 1), (1, 2), (1, 3), (2, 0), (2, 1), (2, 2), (2, 3), (3, 0), (3, 1), (3, 2)}
    for r, c in RB.DEVICE_ENTRIES:
        assert dh[r, c] != RB.SIXDOF_DH[r, c], (r, c)
        other = RB.with_entry(dh, r, c, RB.SIXDOF_DH[r, c])
        moved = {}
        if r == 0:
            moved["seed joints"] = (np.abs(_seed_joints(other, pts) - base_seed).max(), 1e-9)
            mi = 0 if c == 3 else 100
            d = np.abs(O.fabrik_ikine(pts, 1e-3, mi, dh=other)[0] - base_ang[mi])
            moved[f"solved angles, max_iter {mi}"] = (np.nanmax(d), 1e-9)
        elif (r, c) == (3, 3):
            assert np.array_equal(O.fk(th, other)[1], O.fk(th, dh)[1])  # no position moves
            mats = np.array([O.fk_n(other, a) for a in fk_ang])
            moved["mats"] = (np.abs(mats - base_mats).max(), 1e-12)
        else:
            moved["effector"] = (np.abs(O.fk(th, other)[0] - base_xyz).max(), 1e-12)
        if (r, c) in in_jacobian:
            moved["jacobian"] = (np.abs(jacobian(other, th) - base_J).max(),
                                 RB.ANGLE_BOUND[name])
        else:
            assert np.array_equal(jacobian(other, th), base_J), (r, c)
        for what, (d, bound) in moved.items():
            print(f"{name} entry ({r}, {c}): {what} moves by {d:.3g} (bound {bound:.3g})")
            assert d >= 1e6 * bound, (r, c, what, d)


# --------------------------------------------------- refine restatement ----
@pytest.mark.parametrize("name", NAMES)
def test_refine_restatement_converges(name):
    dh = RB.TABLES[name]
    p, _, _ = RB.refine_fixture(dh)
    for tol in (1e-6, 1e-9):
        th, it, err = RB.refine_restated(dh, tol)
        print(f"{name} tol {tol:g}: steps max {it.max()}, mean {it.mean():.3f}; "
              f"max err {err.max():.3g}")
        assert (err <= tol).all() and it.max() <= 20  # no capped row
        assert np.abs(th).max() <= np.pi
        assert np.linalg.norm(O.fk(th, dh)[0] - p, axis=1).max() <= tol + 1e-12


@pytest.mark.parametrize("name", NAMES)
def test_refine_restatement_float64_against_long_double(name):
    """Step counts as tests/test_refine_cpu.py allows them to differ; the angles
    within a factor 2 of the value written into tests/robots.py (libm's last bits
    may differ between machines), and under the ANGLE_BOUND derived from it."""
    dh = RB.TABLES[name]
    for tol, written in zip((1e-6, 1e-9), RB.MEASURED_F64_VS_LONGDOUBLE[name]):
        t64, i64, _ = RB.refine_restated(dh, tol)
        tld, ild, _ = RB.refine_restated(dh, tol, np.longdouble)
        same = i64 == ild
        d = np.abs(t64[same] - tld[same].astype(np.float64)).max()
        print(f"{name} tol {tol:g}: {int((~same).sum())} rows differ in steps; "
              f"max |dtheta| = {d:.3g} (written {written:.3g})")
        assert (np.abs(i64 - ild) <= 1).all() and same.mean() >= 0.999
        assert written / 2 <= d <= 2 * written
        assert d <= RB.ANGLE_BOUND[name]


# ------------------------------------------------------- seed robustness ----
@pytest.mark.parametrize("name", NAMES)
def test_fabrik_ignores_the_seeds_last_bits(name):
    """The kernel's closed-form seed differs from the reference's chain in the last
    bits of x / y.  Every seed's x / y moved by a random -2 .. 2 ulp changes no
    iteration count and moves the final joints by <= 1e-12 on the GPU test's own
    goals: a count mismatch or a 1e-9 miss there is the kernel's."""
    dh = RB.TABLES[name]
    pts = RB.goals(dh)
    assert len(pts) == RB.N_GOALS
    seed = _seed_joints(dh, pts)
    rng = np.random.default_rng(53)
    moved = seed.copy()
    k = rng.integers(-2, 3, size=seed[:, :, :2].shape)
    moved[:, :, :2] += k * np.spacing(np.abs(seed[:, :, :2]))
    assert (moved != seed).mean() > 0.3
    for tol, mi in RB.CONFIGS:
        j0, i0, s0 = O.fabrik_calc(seed, pts, RB.LINKS, tol, mi)
        j1, i1, s1 = O.fabrik_calc(moved, pts, RB.LINKS, tol, mi)
        assert np.array_equal(s0, s1)
        diff = int((i0 != i1).sum())
        fin = np.isfinite(j0).all(axis=(1, 2))
        assert np.array_equal(fin, np.isfinite(j1).all(axis=(1, 2)))
        d = np.abs(j0[fin] - j1[fin]).max()
        print(f"{name} tol {tol:g}: {diff} counts differ, joints move by {d:.3g}")
        assert diff == 0 and d <= 1e-12


def test_goals_cover_the_quadrants_and_the_seed_branches():
    for name, dh in RB.TABLES.items():
        p = RB.goals(dh)
        assert O.check_limits(p, RB.LIMITS) == -1
        q = np.arctan2(p[:, 1], p[:, 0])
        for lo in (-math.pi, -math.pi / 2, 0.0, math.pi / 2):
            assert ((q > lo) & (q < lo + math.pi / 2)).sum() > 1000
        t = p[:, 0] ** 2 + p[:, 1] ** 2
        assert (t < 2.0 ** -1000).sum() >= 20 and np.isnan(p).any(axis=1).sum() == 1


# ---------------------------------------------------------- bad robots ----
def test_out_of_range_robots_in_the_oracle():
    """What the GPU tests of rejected robots expect, from the oracle: alpha_2 = 7
    fails every FABRIK point and every FK row; theta_3 = 7 every FABRIK point (the
    seed pose's own FK) but no FK row; theta_1 is overwritten and never read."""
    pts = RB.goals(RB.GEN_A)[:200]
    ang = np.random.default_rng(3).uniform(-2 * math.pi, 2 * math.pi, (50, 4))
    bad_alpha = RB.with_entry(RB.GEN_A, 3, 1, 7.0)
    assert (O.fabrik_ikine(pts, dh=bad_alpha)[3] == O.E_ANGLE_RANGE).all()
    assert (O.fk(ang, bad_alpha)[2] == O.E_ANGLE_RANGE).all()
    bad_theta = RB.with_entry(RB.GEN_A, 0, 2, 7.0)
    assert (O.fabrik_ikine(pts, dh=bad_theta)[3] == O.E_ANGLE_RANGE).all()
    assert not O.fk(ang, bad_theta)[2].any()
    theta1 = RB.with_entry(RB.GEN_A, 0, 0, 7.0)
    for a, b in zip(O.fabrik_ikine(pts, dh=theta1), O.fabrik_ikine(pts, dh=RB.GEN_A)):
        assert np.array_equal(a, b, equal_nan=True)
