"""ik_analytic_solve without a GPU: the ABI's declarations, the numpy restatement
(kinematics/analytic.py) on the fixtures and edge rows that
tests/test_gpu_analytic.py runs through the kernel, the host unit and the shared row
function in a sanitizer-built stand-alone program (tests/host/analytic_check.cpp),
and the CLI's usage errors."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.test_refine_cpu import N_FIXTURE, SIXDOF_DH, SKEW_DH

CLANGXX = "/opt/rocm/llvm/bin/clang++"  # csrc/Makefile HOSTCXX
CSRC = os.path.join(ROOT, "inversekinematicsann_amd", "csrc")
needs_clang = pytest.mark.skipif(not os.path.exists(CLANGXX),
                                 reason="the ROCm clang++ is not installed")

# d1 0.7, a = [0.3, 1.5, 2.5, 1.0]: a shoulder offset and unequal links
PLANAR2_DH = np.array([[0.0, np.pi / 2, 0.0, 0.0], [0.7, 0.0, 0.0, 0.0], [0.3, 1.5, 2.5, 1.0],
                       [np.pi / 2, 0.0, 0.0, 0.0]])
ROBOTS = {"sixdof": SIXDOF_DH, "planar2": PLANAR2_DH}
ELBOWS = (-1, 1)
N = N_FIXTURE
BOX = ([0.0, -6.0, -3.0], [6.0, 6.0, 6.0])  # SixDOFRobot's workspace

# The restatement's largest FK round trip |O.fk(theta) - p| over fixtures A, B, C and
# the folded edge rows, both robots, both elbows, and the largest |theta_float64 -
# theta_longdouble| over fixture A, as test_restatement_bounds measures them (it
# prints both): 4.51e-15 and 7.56e-15.  The kernel's elementary functions differ from
# libm's in the last units, so it is held to 16 x each -- two orders of magnitude
# below what c3 = (W^2 - a2^2 - a3^2) / (2 a2 a3), s3 = sqrt(1 - c3^2) gives on the
# folded rows (test_textbook_form_is_worse_when_folded).
TRIP_MEASURED = 4.51e-15
ANGLE_MEASURED = 7.56e-15
TRIP_BOUND = 16 * TRIP_MEASURED
ANGLE_BOUND = 16 * ANGLE_MEASURED
# Fixture A's generating angles against the solved ones: the goal carries FK's rounding,
# ~8 eps = 2e-15 on a reach of <= 8, and the pitch 3 eps pi = 2e-15; the elbow's angle
# takes them up by at most 1 / (a_min sin 0.1) = 1 / (1.5 x 0.0998) = 6.7, the other
# angles by as much again: ~3e-14 in all.  Held to 1e-12.
GENERATING_BOUND = 1e-12


def lengths(dh):
    return float(dh[1][0]), *(float(v) for v in dh[2])


def wrap(t):
    return t - 2 * np.pi * np.rint(t / (2 * np.pi))


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def fixtures(robot):
    """{"A": (goals, pitch, theta, sign of theta3), "B": goals, "C": pitches} of one
    robot, from one generator (seed 21) in that order."""
    from oracle import oracle as O
    dh = ROBOTS[robot]
    rng = np.random.default_rng(21)
    n3 = 3 * N
    sign = rng.choice([-1.0, 1.0], n3)
    th = np.stack([rng.uniform(-np.pi / 2, np.pi / 2, n3), rng.uniform(-np.pi, np.pi, n3),
                   sign * rng.uniform(0.1, np.pi - 0.1, n3), rng.uniform(-np.pi, np.pi, n3)],
                  axis=1)
    p = O.fk(th, dh)[0]
    reach = p[:, 0] * np.cos(th[:, 0]) + p[:, 1] * np.sin(th[:, 0]) - lengths(dh)[1]
    keep = np.flatnonzero(reach > 0.05)[:N]
    assert len(keep) == N
    p, th, sign = p[keep].copy(), th[keep].copy(), sign[keep].copy()
    pitch = th[:, 1] + th[:, 2] + th[:, 3]
    box = rng.uniform(BOX[0], BOX[1], (N, 3))
    pr = rng.uniform(-np.pi, np.pi, N)
    return {"A": frozen(p, pitch, th, sign), "B": frozen(box)[0], "C": frozen(pr)[0]}


def edge_goals():
    """SixDOFRobot's edge rows, pitch None: (goals, fails).  Rows 5..12 are folded
    (the wrist within 1e-4 of the shoulder)."""
    rng = np.random.default_rng(22)
    rows = [[6.0, 0.0, 2.0], [0.0, 0.0, 2.0], [0.0, 0.0, 8.0], [0.0, 0.0, -4.0], [7.0, 0.0, 2.0],
            [2.0, 0.0, 2.0]]
    for off in (0.0, 1e-12, -1e-12, 1e-9, -1e-9, 1e-6, -1e-4):
        az, el = rng.uniform(-1.5, 1.5), rng.uniform(-1.5, 1.5)
        rho = 2.0 + off
        rows.append([rho * np.cos(el) * np.cos(az), rho * np.cos(el) * np.sin(az),
                     2.0 + rho * np.sin(el)])
    rows.append([np.nan, 1.0, 1.0])
    goals = np.array(rows)
    fails = np.zeros(len(rows), bool)
    fails[[4, len(rows) - 1]] = True
    return goals, fails


EDGE_FOLDED = slice(5, 13)
# rows with a pitch of their own: (goal, pitch, fails strict, fails nearest, moved)
EDGE_PITCH = [([4.0, 0.0, 2.0], 0.0, False, False, False),
              ([4.0, 0.0, 2.0], np.nan, True, True, False),
              ([4.0, 0.0, 2.0], np.inf, True, True, False),
              ([5.5, 0.0, 2.0], 3.0, True, False, True),
              ([5.5, 0.0, 2.0], 0.25 + 4 * np.pi, False, False, False),
              ([7.0, 0.0, 2.0], 0.0, True, True, False)]


@functools.lru_cache(maxsize=None)
def reference(robot, fixture, elbow, nearest, dtype=np.float64):
    """analytic_reference on a fixture ("A": its own pitches, strict or nearest; "B":
    the box, pitch None; "C": fixture A's goals at random pitches), computed once."""
    from inversekinematicsann_amd.kinematics.analytic import analytic_reference
    f = fixtures(robot)
    p, pitch = {"A": (f["A"][0], f["A"][1]), "B": (f["B"], None), "C": (f["A"][0], f["C"])}[fixture]
    return frozen(*analytic_reference(p, pitch, elbow, nearest, ROBOTS[robot], dtype=dtype))


def box_fails(robot):
    """Which of fixture B's goals no pitch reaches, and their distance from the two
    spheres that decide it."""
    d1, a1, a2, a3, a4 = lengths(ROBOTS[robot])
    q = fixtures(robot)["B"]
    rho = np.hypot(np.hypot(q[:, 0], q[:, 1]) - a1, q[:, 2] - d1)
    outer, inner = a2 + a3 + a4, max(abs(a2 - a3) - a4, 0.0)
    gap = min(np.abs(rho - outer).min(), np.abs(rho - inner).min() if inner > 0 else np.inf)
    return (rho > outer) | (rho < inner), gap


def round_trip(ang, p, dh, ok):
    from oracle import oracle as O
    return np.linalg.norm(O.fk(ang[ok], dh)[0] - p[ok], axis=1)


def check_rows(ang, used, failed, p, elbow, dh, bound):
    """What every solved batch must satisfy; returns the largest round trip."""
    ok = ~failed
    assert np.isnan(ang[failed]).all() and np.isnan(used[failed]).all()
    assert np.isfinite(ang[ok]).all() and np.isfinite(used[ok]).all()
    assert np.abs(ang[ok]).max() <= np.pi
    assert (ang[ok, 2] * elbow >= 0).all()
    trip = round_trip(ang, p, dh, ok)
    assert trip.max() <= bound, trip.max()
    dev = np.abs(wrap(ang[ok, 1] + ang[ok, 2] + ang[ok, 3] - used[ok])).max()
    # three angles of <= pi and the pitch, each rounded once, and wrap's product
    assert dev <= 8 * np.pi * np.finfo(np.float64).eps, dev
    return trip.max()


# 1 ---------------------------------------------------------------------------
def test_symbol_and_enums_declared_and_exported():
    from inversekinematicsann_amd import _native
    hdr = open(os.path.join(ROOT, "include", "ikhip.h")).read()
    assert re.search(r"^int ik_analytic_solve\(ik_ctx \*ctx,", hdr, re.M)
    assert re.search(r"enum \{ IK_ELBOW_UP = -1, IK_ELBOW_DOWN = 1 \};", hdr)
    assert re.search(r"IK_F_PITCH_NEAREST = 8\b", hdr)
    assert "ik_analytic_solve" in _native.EXPORTED_SYMBOLS
    assert (_native.IK_ELBOW_UP, _native.IK_ELBOW_DOWN, _native.IK_F_PITCH_NEAREST) == (-1, 1, 8)


# 2 ---------------------------------------------------------------------------
@pytest.mark.parametrize("elbow", ELBOWS)
@pytest.mark.parametrize("robot", list(ROBOTS))
def test_restatement_fixture_a(robot, elbow):
    p, pitch, th, sign = fixtures(robot)["A"]
    dh = ROBOTS[robot]
    for nearest in (False, True):
        ang, used, failed, moved = reference(robot, "A", elbow, nearest)
        assert not failed.any() and not moved.any()  # no row is left out below
        assert used.tobytes() == pitch.tobytes()
        check_rows(ang, used, failed, p, elbow, dh, TRIP_BOUND)
    own = sign == elbow
    assert 0.4 < own.mean() < 0.6
    d = np.abs(wrap(ang[own] - th[own])).max()
    print(f"{robot} elbow {elbow}: max |theta - generating theta| = {d:.3g} on {own.sum()} rows")
    assert d <= GENERATING_BOUND


@pytest.mark.parametrize("robot", list(ROBOTS))
def test_restatement_fixture_b(robot):
    q = fixtures(robot)["B"]
    want, gap = box_fails(robot)
    print(f"{robot}: {want.sum()} of {N} box goals out of reach, nearest sphere {gap:.3g} away")
    assert gap >= 1e-6 and 0 < want.sum() < N
    for elbow in ELBOWS:
        ang, used, failed, moved = reference(robot, "B", elbow, True)
        assert np.array_equal(failed, want)
        check_rows(ang, used, failed, q, elbow, ROBOTS[robot], TRIP_BOUND)
        sang, sused, sfailed, smoved = reference(robot, "B", elbow, False)
        assert not smoved.any() and np.array_equal(sfailed, failed | moved)
        keep = ~moved
        assert ang[keep].tobytes() == sang[keep].tobytes()
        print(f"{robot} elbow {elbow}: {moved.sum()} pitches moved")
        if robot == "planar2":  # gamma itself folds the unequal links too far
            assert moved.sum() > 0
        else:
            assert moved.sum() == 0


@pytest.mark.parametrize("elbow", ELBOWS)
@pytest.mark.parametrize("robot", list(ROBOTS))
def test_restatement_fixture_c(robot, elbow):
    p, pr = fixtures(robot)["A"][0], fixtures(robot)["C"]
    ang0, used0, failed0, moved0 = reference(robot, "C", elbow, False)
    ang1, used1, failed1, moved1 = reference(robot, "C", elbow, True)
    print(f"{robot} elbow {elbow}: {failed0.sum()} of {N} random pitches infeasible")
    assert 0.2 * N < failed0.sum() < 0.6 * N and not moved0.any()
    assert not failed1.any() and np.array_equal(moved1, failed0)
    keep = ~moved1
    assert ang0[keep].tobytes() == ang1[keep].tobytes()
    assert used0[keep].tobytes() == used1[keep].tobytes() == pr[keep].tobytes()
    for ang, used, failed in ((ang0, used0, failed0), (ang1, used1, failed1)):
        check_rows(ang, used, failed, p, elbow, ROBOTS[robot], TRIP_BOUND)
    # a moved pitch stays on its own side of gamma and is the nearer end: no other
    # feasible pitch lies between it and the one asked for
    from inversekinematicsann_amd.kinematics.analytic import analytic_reference
    mid = pr[moved1] + 0.5 * wrap(used1[moved1] - pr[moved1])
    assert analytic_reference(p[moved1], mid, elbow, False, ROBOTS[robot])[2].all()


@pytest.mark.parametrize("elbow", ELBOWS)
def test_restatement_edge_rows(elbow):
    from inversekinematicsann_amd.kinematics.analytic import analytic_reference
    goals, fails = edge_goals()
    for nearest in (False, True):
        ang, used, failed, moved = analytic_reference(goals, None, elbow, nearest, SIXDOF_DH)
        assert np.array_equal(failed, fails) and not moved.any()
        check_rows(ang, used, failed, goals, elbow, SIXDOF_DH, TRIP_BOUND)
    assert np.array_equal(ang[0], [0.0, 0.0, 0.0, 0.0])  # full stretch
    assert np.array_equal(ang[5], [0.0, 0.0, elbow * np.pi, -elbow * np.pi])  # folded
    p = np.array([r[0] for r in EDGE_PITCH])
    ph = np.array([r[1] for r in EDGE_PITCH])
    for nearest in (False, True):
        ang, used, failed, moved = analytic_reference(p, ph, elbow, nearest, SIXDOF_DH)
        assert failed.tolist() == [r[3 if nearest else 2] for r in EDGE_PITCH]
        assert moved.tolist() == [r[4] and nearest for r in EDGE_PITCH]
        check_rows(ang, used, failed, p, elbow, SIXDOF_DH, TRIP_BOUND)
        keep = ~failed & ~moved
        assert used[keep].tobytes() == ph[keep].tobytes()


# 3 ---------------------------------------------------------------------------
def folded_trips(elbow):
    from inversekinematicsann_amd.kinematics.analytic import analytic_reference
    goals, fails = edge_goals()
    g = goals[EDGE_FOLDED]
    ang, _, failed, _ = analytic_reference(g, None, elbow, False, SIXDOF_DH)
    return g, ang, round_trip(ang, g, SIXDOF_DH, ~failed)


def test_restatement_bounds():
    """Measures TRIP_MEASURED and ANGLE_MEASURED (printed) and checks the values written
    above against them."""
    trip, dang = 0.0, 0.0
    for robot, dh in ROBOTS.items():
        f = fixtures(robot)
        for elbow in ELBOWS:
            for fx, p, modes in (("A", f["A"][0], (False,)), ("B", f["B"], (True,)),
                                 ("C", f["A"][0], (False, True))):
                for nearest in modes:
                    ang, _, failed, _ = reference(robot, fx, elbow, nearest)
                    trip = max(trip, round_trip(ang, p, dh, ~failed).max())
            a64 = reference(robot, "A", elbow, False)[0]
            ald, _, fld, _ = reference(robot, "A", elbow, False, np.longdouble)
            assert not fld.any()
            dang = max(dang, np.abs(a64 - ald.astype(np.float64)).max())
    for elbow in ELBOWS:
        trip = max(trip, folded_trips(elbow)[2].max())
    print(f"largest round trip {trip:.3g}; largest |theta_f64 - theta_longdouble| {dang:.3g}")
    # numpy's sin / cos / arctan2 differ in the last unit between CPUs (its SIMD
    # dispatch): the written values are held to a factor 2 either way
    assert TRIP_MEASURED / 2 <= trip <= 2 * TRIP_MEASURED
    assert ANGLE_MEASURED / 2 <= dang <= 2 * ANGLE_MEASURED


def test_textbook_form_is_worse_when_folded():
    """c3 from W^2 and s3 = sqrt(1 - c3^2) on the folded rows: the round trip the
    kernel's bound is two orders of magnitude below."""
    g, _, trips = folded_trips(1)
    d1, a1, a2, a3, a4 = lengths(SIXDOF_DH)
    r, h = np.hypot(g[:, 0], g[:, 1]) - a1, g[:, 2] - d1
    phi = np.arctan2(h, r)
    wr, wh = r - a4 * np.cos(phi), h - a4 * np.sin(phi)
    c3 = np.clip((wr * wr + wh * wh - a2 * a2 - a3 * a3) / (2 * a2 * a3), -1, 1)
    s3 = np.sqrt(1 - c3 * c3)
    t3 = np.arctan2(s3, c3)
    t2 = np.arctan2(wh, wr) - np.arctan2(a3 * s3, a2 + a3 * c3)
    ang = np.stack([np.arctan2(g[:, 1], g[:, 0]), t2, t3, phi - t2 - t3], axis=1)
    worst = round_trip(ang, g, SIXDOF_DH, np.ones(len(g), bool)).max()
    print(f"folded rows: textbook form {worst:.3g}, factored form {trips.max():.3g}")
    assert worst >= 100 * TRIP_BOUND and trips.max() <= 2 * TRIP_MEASURED


def test_planar_robot_rule():
    from inversekinematicsann_amd.kinematics.analytic import planar_robot
    assert planar_robot(SIXDOF_DH) == (2.0, 0.0, 2.0, 2.0, 2.0)
    assert planar_robot(PLANAR2_DH) == (0.7, 0.3, 1.5, 2.5, 1.0)
    with pytest.raises(ValueError, match="^alpha2 = 0.4 must be 0"):
        planar_robot(SKEW_DH)
    for (i, j), v, name in (((3, 0), -np.pi / 2, "alpha1"), ((3, 0), np.nan, "alpha1"),
                            ((3, 3), 1e-9, "alpha4"), ((1, 2), 0.3, "d3"), ((2, 1), 0.0, "a2"),
                            ((2, 2), np.inf, "a3"), ((2, 3), np.nan, "a4"), ((2, 0), -0.1, "a1")):
        dh = SIXDOF_DH.copy()
        dh[i, j] = v
        with pytest.raises(ValueError, match=f"^{name} = "):
            planar_robot(dh)


# 4 ---------------------------------------------------------------------------
@needs_clang
def test_analytic_check_program(tmp_path):
    """The host unit's acceptance table and the row function the kernel compiles, in a
    stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer; its rows
    against the restatement (numpy's and libm's functions differ in the last units:
    the same pattern of failed / moved rows, the round trip within the kernel's bound,
    the pitch used bit-equal where it was not moved)."""
    from inversekinematicsann_amd.kinematics.analytic import analytic_reference
    exe = os.path.join(str(tmp_path), "analytic_check")
    subprocess.run([CLANGXX, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", CSRC,
                    os.path.join(ROOT, "tests", "host", "analytic_check.cpp"),
                    os.path.join(CSRC, "ik_analytic_plan.cpp"), "-o", exe], check=True)
    goals, _ = edge_goals()
    cases = []  # (dh, goals, pitch or None, elbow, nearest)
    for elbow in ELBOWS:
        for nearest in (False, True):
            cases.append((SIXDOF_DH, goals, None, elbow, nearest))
            cases.append((SIXDOF_DH, np.array([r[0] for r in EDGE_PITCH]),
                          np.array([r[1] for r in EDGE_PITCH]), elbow, nearest))
            for robot, dh in ROBOTS.items():
                cases.append((dh, fixtures(robot)["A"][0][:64], fixtures(robot)["C"][:64], elbow,
                              nearest))
    rows = tmp_path / "rows.txt"
    with open(rows, "w") as f:
        for dh, p, ph, elbow, nearest in cases:
            for i in range(len(p)):
                vals = [*lengths(dh), *p[i], 0.0 if ph is None else 1.0,
                        0.0 if ph is None else ph[i], float(elbow), float(nearest)]
                f.write(" ".join(repr(float(v)) for v in vals) + "\n")
    r = subprocess.run([exe, str(rows)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "analytic_check ok" in r.stdout, r.stdout[-4000:]
    got = np.array([[float(v) for v in line.split()[1:]] for line in r.stdout.splitlines()
                    if line.startswith("row ")])
    at = 0
    for dh, p, ph, elbow, nearest in cases:
        g = got[at:at + len(p)]
        at += len(p)
        ang, used, failed, moved = analytic_reference(p, ph, elbow, nearest, dh)
        assert np.array_equal(g[:, 5] != 0, failed) and np.array_equal(g[:, 6] != 0, moved)
        check_rows(g[:, :4], g[:, 4], failed, p, elbow, dh, TRIP_BOUND)
        keep = ~failed & ~moved
        assert g[keep, 4].tobytes() == used[keep].tobytes()
    assert at == len(got) and f"rows {at}" in r.stdout


# 5 ---------------------------------------------------------------------------
def cli_error(argv, capsys):
    from inversekinematicsann_amd.cli import main
    with pytest.raises(SystemExit) as ei:
        main(argv)
    assert ei.value.code == 2
    return capsys.readouterr().err


def test_cli_usage_errors(tmp_path, capsys):
    from inversekinematicsann_amd.cli import EXAMPLES, main
    pts = tmp_path / "p.csv"
    pts.write_text("x,y,z\n3.0,0.0,2.0\n")
    base = ["--inverse-kine", "--points", str(pts)]
    for flag in (["--pitch", "0.5"], ["--elbow", "down"], ["--nearest-pitch"]):
        err = cli_error(base + ["--method", "fabrik"] + flag, capsys)
        assert f"{flag[0]} is only valid with --method analytic" in err
    assert "--pitch is only valid" in cli_error(
        base + ["--method", "ann", "--model", "m.npz", "--pitch", "0"], capsys)
    assert "invalid choice" in cli_error(base + ["--method", "analytic", "--elbow", "left"], capsys)
    assert "--points" in cli_error(["--inverse-kine", "--method", "analytic"], capsys)
    four = tmp_path / "p4.csv"
    four.write_text("x,y,z,pitch\n3.0,0.0,2.0,0.1\n")
    err = cli_error(["--inverse-kine", "--method", "analytic", "--points", str(four), "--pitch",
                     "0.2"], capsys)
    assert "--pitch is not valid with a points file that has a pitch column" in err
    assert main(["--inverse-kine", "--method", "analytic", "--example"]) == 0
    assert capsys.readouterr().out.strip() == EXAMPLES["analytic"]
