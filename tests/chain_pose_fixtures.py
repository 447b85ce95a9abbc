"""Pose goals, seeds and restated results that tests/test_chain_pose_cpu.py and
tests/test_gpu_chain_pose.py share, on the DH tables of tests/chain_fixtures.py.

A goal is (p, G) = the translation and the rotation of the product of the nj 4 x 4 DH
matrices at theta*, formed in long double and rounded to float64; the seeds are 0.05 rad
off.  nj = 3 is the over-determined problem (6 rows, 3 joints), 6 the square one, 7 and
8 the redundant ones.

The kernel is compared with the restatement (kinematics/chain.py chain_pose_reference)
on the stable rows only: those on which the float64 and the long-double restatement
both converge, in equal step counts.  tests/test_chain_pose_cpu.py asserts that at least
99.5 % of every fixture's rows are stable."""
import functools

import numpy as np

from tests import chain_fixtures as F

NJS = (3, 6, 7, 8)
N_ROWS = F.N_ROWS
DAMPING = F.DAMPING
TOLS = (1e-6, 1e-9)
ROT_WEIGHT = 1.0
# steps an attempt: plain damped least squares needs more of them near the singular
# poses of the square problem (6 joints) than the position solve's 30
MAX_ITER = {3: 30, 6: 60, 7: 30, 8: 30}
STABLE_SHARE = 0.995


def pose_longdouble(dh, ang):
    """(p n x 3, R n x 3 x 3) of the product of the nj 4 x 4 matrices Rz(theta) Tz(d)
    Tx(a) Rx(alpha) in long double.  Shares nothing with the library or its
    restatement."""
    dh = np.asarray(dh, np.longdouble)
    th = np.asarray(ang, np.longdouble).reshape(-1, dh.shape[1])
    n = th.shape[0]
    M = np.tile(np.identity(4, np.longdouble), (n, 1, 1))
    for i in range(dh.shape[1]):
        A = np.tile(np.identity(4, np.longdouble), (n, 1, 1))
        ct, st = np.cos(th[:, i]), np.sin(th[:, i])
        ca, sa = np.cos(dh[3, i]), np.sin(dh[3, i])
        A[:, 0, 0], A[:, 0, 1], A[:, 0, 2], A[:, 0, 3] = ct, -st * ca, st * sa, dh[2, i] * ct
        A[:, 1, 0], A[:, 1, 1], A[:, 1, 2], A[:, 1, 3] = st, ct * ca, -ct * sa, dh[2, i] * st
        A[:, 2, 1], A[:, 2, 2], A[:, 2, 3] = sa, ca, dh[1, i]
        M = np.einsum("nij,njk->nik", M, A)
    return M[:, :3, 3], M[:, :3, :3]


def chord(R, G):
    """sqrt(1/2 |R - G|_F^2) per row: 2 sin(phi / 2) between two rotations."""
    d = (np.asarray(R) - np.asarray(G)).reshape(len(R), -1)
    return np.sqrt(0.5 * (d * d).sum(axis=1))


def _frozen(out):
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def pose_fixture(nj):
    """(p n x 3, G n x 3 x 3, seeds n x nj, theta* n x nj) of table(nj)."""
    rng = np.random.default_rng(300 + nj)
    th = rng.uniform(-np.pi / 2, np.pi / 2, (N_ROWS, nj))
    p, G = pose_longdouble(F.table(nj), th)
    sd = th + rng.normal(0, 0.05, (N_ROWS, nj))
    return _frozen((p.astype(np.float64), G.astype(np.float64), sd, th))


@functools.lru_cache(maxsize=None)
def restated(nj, tol, dtype=np.float64):
    """chain_pose_reference on pose_fixture(nj) at tol = rot_tol: (theta, iters, tries,
    ep, er)."""
    from inversekinematicsann_amd.kinematics.chain import chain_pose_reference
    p, G, sd, _ = pose_fixture(nj)
    return _frozen(chain_pose_reference(p, G, sd, tol, tol, ROT_WEIGHT, MAX_ITER[nj], DAMPING,
                                        F.table(nj), dtype=dtype))


def _stable(r64, rld, tol, rot_tol):
    conv = (r64[3] <= tol) & (r64[4] <= rot_tol) & (rld[3] <= tol) & (rld[4] <= rot_tol)
    return conv & (r64[1] == rld[1])


@functools.lru_cache(maxsize=None)
def stable(nj, tol):
    """The rows on which the float64 and the long-double restatement both converge with
    equal step counts."""
    s = _stable(restated(nj, tol), restated(nj, tol, np.longdouble), tol, tol)
    s.setflags(write=False)
    return s


# max |theta_f64 - theta_longdouble| of the restatement on the stable rows of
# pose_fixture(nj) at tol 1e-6 and 1e-9; measured and asserted by
# tests/test_chain_pose_cpu.py::test_stable_rows_and_float64_against_long_double.  The
# kernel's sincos_fk adds rounding of the same order: it is held to 10 x the value.
MEASURED_F64_VS_LONGDOUBLE = {
    3: (4.00e-15, 6.67e-16),
    6: (5.23e-13, 1.25e-13),
    7: (2.43e-12, 2.43e-12),
    8: (8.71e-14, 8.59e-14),
}
ANGLE_BOUND = {k: 10 * max(v) for k, v in MEASURED_F64_VS_LONGDOUBLE.items()}

# Limits at 7 joints that bind: joint 1 free, joints 2..7 the interval theta* was drawn
# from, so every goal is reachable inside them and seeds 0.05 rad off start outside.
LIMITS7 = (np.array([-np.inf] + [-np.pi / 2] * 6), np.array([np.inf] + [np.pi / 2] * 6))
for _a in LIMITS7:
    _a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def restated_limited7(dtype=np.float64):
    """chain_pose_reference on pose_fixture(7) under LIMITS7 at tol = rot_tol = 1e-9."""
    from inversekinematicsann_amd.kinematics.chain import chain_pose_reference
    p, G, sd, _ = pose_fixture(7)
    return _frozen(chain_pose_reference(p, G, sd, 1e-9, 1e-9, ROT_WEIGHT, MAX_ITER[7], DAMPING,
                                        F.table(7), LIMITS7, dtype=dtype))


@functools.lru_cache(maxsize=None)
def stable_limited7():
    s = _stable(restated_limited7(), restated_limited7(np.longdouble), 1e-9, 1e-9)
    s.setflags(write=False)
    return s


# The same under LIMITS7, on its stable rows; asserted by the same CPU test.
MEASURED_LIMITED7_F64_VS_LONGDOUBLE = 7.41e-12
LIMITED7_ANGLE_BOUND = 10 * MEASURED_LIMITED7_F64_VS_LONGDOUBLE

# Restarts from the home pose at 7 joints: pose goals of uniform angles, tol = rot_tol =
# 1e-6, HOME_ITER steps an attempt.
HOME_NJ = 7
HOME_ROWS = 600
HOME_ITER = 40
HOME_RESTARTS = 2


@functools.lru_cache(maxsize=None)
def home_fixture():
    rng = np.random.default_rng(400 + HOME_NJ)
    th = rng.uniform(-np.pi, np.pi, (HOME_ROWS, HOME_NJ))
    p, G = pose_longdouble(F.table(HOME_NJ), th)
    return _frozen((p.astype(np.float64), G.astype(np.float64)))


@functools.lru_cache(maxsize=None)
def home_restated(restarts):
    from inversekinematicsann_amd.kinematics.chain import chain_pose_reference
    p, G = home_fixture()
    return _frozen(chain_pose_reference(p, G, None, 1e-6, 1e-6, ROT_WEIGHT, HOME_ITER, DAMPING,
                                        F.table(HOME_NJ), restarts=restarts))


# Rows of home_fixture() the restatement leaves unconverged with no restart and with
# HOME_RESTARTS; asserted by tests/test_chain_pose_cpu.py::test_restarts_reduce_capped.
HOME_CAPPED = (40, 2)
