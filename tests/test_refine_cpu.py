"""The damped-least-squares refine without a GPU: the ABI's declarations, the
analytic Jacobian against central differences of the oracle's FK, and the numpy
restatement (kinematics/refine.py) on the fixture and the edge rows that
tests/test_gpu_refine.py runs through the kernel."""
import functools
import os
import re

import numpy as np

from tests.conftest import ROOT

SIXDOF_DH = np.array([[0.0, np.pi / 2, 0.0, 0.0], [2.0, 0.0, 0.0, 0.0], [0.0, 2.0, 2.0, 2.0],
                      [np.pi / 2, 0.0, 0.0, 0.0]])
# a chain with a twist at joint 2 and an offset at joint 3 (rows: theta, d, a, alpha)
SKEW_DH = np.array([[0.0, np.pi / 2, 0.0, 0.0], [2.0, 0.0, 0.3, 0.0], [0.0, 2.0, 2.0, 2.0],
                    [np.pi / 2, 0.4, 0.0, 0.0]])
N_FIXTURE = 64 * 64 + 37


@functools.lru_cache(maxsize=None)
def fixture(n=N_FIXTURE):
    """(goals n x 3, seeds n x 4, theta* n x 4): reachable goals with seeds 0.05 rad
    off.  About 20 % of the goals lie outside SixDOFRobot's workspace box."""
    from oracle import oracle as O
    rng = np.random.default_rng(7)
    th = np.stack([rng.uniform(-np.pi / 2, np.pi / 2, n), rng.uniform(0, np.pi / 2, n),
                   rng.uniform(-np.pi / 2, 0, n), rng.uniform(-np.pi / 2, np.pi / 2, n)], axis=1)
    p = O.fk(th)[0]
    seed = th + rng.normal(0, 0.05, (n, 4))
    for a in (p, seed, th):
        a.setflags(write=False)
    return p, seed, th


@functools.lru_cache(maxsize=None)
def reference(tol, max_iter=20, dtype=np.float64):
    """refine_reference on the fixture, computed once per (tol, max_iter, dtype)."""
    from inversekinematicsann_amd.kinematics.refine import refine_reference
    p, seed, _ = fixture()
    out = refine_reference(p, seed, tol, max_iter, 1e-3, SIXDOF_DH, dtype=dtype)
    for a in out:
        a.setflags(write=False)
    return out


def test_symbols_declared_and_exported():
    from inversekinematicsann_amd import _native
    hdr = open(os.path.join(ROOT, "include", "ikhip.h")).read()
    for sym in ("ik_refine", "ik_ann_solve_refined"):
        assert re.search(rf"^int {sym}\(ik_ctx \*ctx,", hdr, re.M), sym
        assert sym in _native.EXPORTED_SYMBOLS, sym


def test_jacobian_matches_central_differences():
    """h = 1e-5: truncation h^2 / 6 |f'''| <= 1e-10 / 6 * 8 (total link length),
    rounding ~ eps * 8 / h ~ 2e-10; both well under 1e-8."""
    from inversekinematicsann_amd.kinematics.refine import jacobian
    from oracle import oracle as O
    rng = np.random.default_rng(11)
    th = rng.uniform(-np.pi, np.pi, (256, 4))
    h = 1e-5
    for dh in (SIXDOF_DH, SKEW_DH):
        J = jacobian(dh, th)
        assert J.shape == (256, 3, 4) and J.dtype == np.float64
        for i in range(4):
            d = np.zeros(4)
            d[i] = h
            fd = (O.fk(th + d, dh)[0] - O.fk(th - d, dh)[0]) / (2 * h)
            worst = np.abs(J[:, :, i] - fd).max()
            print(f"joint {i + 1}: max |J - central difference| = {worst:.3g}")
            assert worst <= 1e-8


def test_restatement_converges_on_fixture():
    from oracle import oracle as O
    p, _, _ = fixture()
    th, it, err = reference(1e-9)
    print(f"steps: max {it.max()}, mean {it.mean():.3f}; max err {err.max():.3g}")
    assert (err <= 1e-9).all() and it.max() <= 20
    assert np.abs(th).max() <= np.pi
    assert np.linalg.norm(O.fk(th)[0] - p, axis=1).max() <= 1e-9 + 1e-12


# How far float64's own rounding moves the converged angles: max |theta_f64 -
# theta_longdouble| of refine_reference over the fixture's rows with equal step
# counts (all 4133), measured by test_restatement_float64_against_long_double:
# 5.40e-14 at tol 1e-6, 5.62e-14 at tol 1e-9.  The kernel's sincos_fk adds rounding
# of the same order, so its angles are held to 10 x the measured value.
MEASURED_F64_VS_LONGDOUBLE = 5.62e-14
ANGLE_BOUND = 10 * MEASURED_F64_VS_LONGDOUBLE


def test_restatement_float64_against_long_double():
    """The rounding of float64 does not move the step counts, and moves the angles
    by the measured value above (printed; held here to the kernel's bound)."""
    for tol in (1e-6, 1e-9):
        t64, i64, _ = reference(tol)
        tld, ild, _ = reference(tol, 20, np.longdouble)
        same = i64 == ild
        d = np.abs(t64[same] - tld[same].astype(np.float64)).max()
        print(f"tol {tol:g}: {int((~same).sum())} rows differ in steps; max |dtheta| = {d:.3g}")
        assert (np.abs(i64 - ild) <= 1).all() and same.mean() >= 0.999
        assert d <= ANGLE_BOUND


def test_restatement_edge_rows():
    from inversekinematicsann_amd.kinematics.refine import refine_reference, wrap
    z = np.zeros((1, 4))
    th, it, err = refine_reference([[0.0, 0.0, 5.0]], z, 1e-9, 30, 1e-3, SIXDOF_DH)
    assert err[0] <= 1e-9 and it[0] <= 30
    th, it, err = refine_reference([[6.0, 6.0, 6.0]], z, 1e-9, 30, 1e-3, SIXDOF_DH)
    assert it[0] == 30 and err[0] > 1e-9 and np.isfinite(th).all()
    seed = np.array([[0.1, 7.0, -0.3, -9.5]])
    th, it, err = refine_reference([[np.nan, 1.0, 1.0]], seed, 1e-9, 30, 1e-3, SIXDOF_DH)
    assert it[0] == 0 and np.isnan(err[0]) and np.array_equal(th, wrap(seed))
    # the documented limit: a goal on the line of a fully stretched seed stays put
    th, it, err = refine_reference([[3.0, 0.0, 2.0]], z, 1e-9, 30, 1e-3, SIXDOF_DH)
    assert it[0] == 30 and abs(err[0] - 3.0) <= 1e-6 and np.isfinite(th).all()
