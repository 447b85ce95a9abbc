"""The FABRIK loop condition's error band (csrc/ik_fabrik_step.h, fabrik_step4_lazy;
csrc/ik_fabrik_plan.cpp, fabrik_band), checked numerically on the CPU: along real
FABRIK iterations (numpy float64, the reference's arithmetic: kinematics/point.py:25-45, fabrik.py:19-64),
the start and goal errors the step approximates from its radicands' roots,
|sqrt(x) - L0| and |sqrt(x3) - L3| (r06; r05: |1 - q| sqrt(x)), stay within the band's
D of the reference's own
|B0 - start| and |F3 - goal|, and the band's decisions agree with the exact
comparison for thresholds placed right at the errors.  The GPU tests check the
kernel bit for bit; this pins the bound the kernel's proof rests on, including the
converged states where the errors are tiny and the approximation is all roundoff.
band() below restates fabrik_band (csrc/ik_fabrik_plan.cpp); the check program
tests/host/fabrik_plan_check.cpp prints the function's own results (--band), and
band() must reproduce them bit for bit, so the experiments run on the source's band.
"""
import math

import numpy as np
import pytest

from tests.test_fabrik_plan_cpu import build_check, run_check

U = 2.0 ** -53


def pb(s, e, d):
    """get_point_between(s, e, d) and its radicand / quotient, batched."""
    dv = e - s
    x = (dv[:, 0] * dv[:, 0] + dv[:, 1] * dv[:, 1]) + dv[:, 2] * dv[:, 2]
    q = d / np.sqrt(x)
    return s + q[:, None] * dv, x, q


def band(tol2, n1max, sum_l):
    """fabrik_band (ik_fabrik_plan.cpp), restated (test_band_restates_the_source)."""
    if not tol2 > 0.0:
        return -1.0, np.inf, 0.0  # decides nothing: every comparison exact
    T = np.sqrt(tol2)
    tlo, thi = T * (1.0 - 2.0 ** -50), T * (1.0 + 2.0 ** -50)
    d = 2.0 ** -52 * (6.0 * n1max + 8.0 * sum_l + 1.0)
    hi = (d + thi) * (1.0 + 2.0 ** -36)
    lo = (tlo - d) * (1.0 - 2.0 ** -36) if d <= 0.5 * tlo else -1.0
    return lo, hi, d


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    """The check program's verdict on ik_fabrik_plan.cpp (its own assertions all
    held) and its --band lines: (tol2, n1max, sum_l, lo, hi) from fabrik_band itself."""
    exe = build_check(tmp_path_factory.mktemp("fabrik_plan"))
    assert "fabrik_plan_check ok" in run_check(exe)
    rows = [tuple(float.fromhex(v) for v in line.split())
            for line in run_check(exe, "--band").splitlines()]
    assert len(rows) >= 30 and all(len(r) == 5 for r in rows)
    return rows


def test_band_restates_the_source(plan_check):
    """band() gives fabrik_band's lo and hi bit for bit on the program's list: the
    thresholds of tol 1e-3 / 1e-5 / 1e-13 (and others down to the smallest subnormal
    and up to DBL_MAX), n1max of the default launch, of a small and a large robot and
    -1 ("no lane"), and tol2 <= 0 / NaN."""
    bits = lambda v: np.float64(v).tobytes()
    n1s, decided, undecided = set(), 0, 0
    for tol2, n1max, sum_l, lo, hi in plan_check:
        plo, phi, _ = band(tol2, n1max, sum_l)
        assert bits(plo) == bits(lo) and bits(phi) == bits(hi), (tol2.hex(), n1max, sum_l)
        n1s.add(n1max)
        decided += lo > 0.0
        undecided += lo == -1.0
    assert -1.0 in n1s and 64.0 * 11.0 in n1s
    assert decided >= 10 and undecided >= 10  # both branches of lo


def chains(n, rng):
    start = np.tile([0.0, 0.0, 2.0], (n, 1))
    J = [start]
    for _ in range(3):
        u = rng.normal(size=(n, 3))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        J.append(J[-1] + 2.0 * u)
    g = start + rng.uniform(-7.5, 7.5, size=(n, 3))
    return J, g


def test_band_bounds_the_approximate_errors():
    rng = np.random.default_rng(5)
    L = 2.0
    n = 20000
    J, g = chains(n, rng)
    start, c1, c2 = J[0], J[1], J[2]
    n1 = np.abs(start).sum(1) + np.abs(g).sum(1)
    worst = 0.0
    for it in range(80):
        b2, _, _ = pb(g, c2, L)
        b1, _, _ = pb(b2, c1, L)
        b0, x, q = pb(b1, start, L)
        se = np.sqrt(((b0 - start) ** 2).sum(1))
        sea = np.abs(np.sqrt(x) - L)
        c1, _, _ = pb(start, b1, L)
        c2, _, _ = pb(c1, b2, L)
        c3, x3, cq = pb(c2, g, L)
        ge = np.sqrt(((c3 - g) ** 2).sum(1))
        gea = np.abs(np.sqrt(x3) - L)
        d = 2.0 ** -52 * (6.0 * n1 + 8.0 * 4 * L + 1.0)
        ok = np.isfinite(se) & np.isfinite(ge)
        # the kernel's D is twice the bound it needs; the observed gap stays below half
        r = np.maximum(np.abs(se - sea), np.abs(ge - gea))[ok] / d[ok]
        worst = max(worst, float(r.max()))
        assert (r <= 0.5).all(), (it, float(r.max()))
    assert worst > 0.0  # the comparison did see roundoff


def test_band_decisions_match_exact_comparisons():
    """Thresholds from 1e-6 relative down to one ulp around the errors themselves:
    wherever the band decides, it decides as the exact squared comparison does (and
    the thresholds closest to the error are left to the exact comparison).  The
    approximation is the kernel's root-space one, |sqrt(x) - L0|, against the
    un-squared band; the exact comparison is the squared one."""
    rng = np.random.default_rng(6)
    L = 2.0
    J, g = chains(4000, rng)
    start, c1, c2 = J[0], J[1], J[2]
    n1max = float((np.abs(start).sum(1) + np.abs(g).sum(1)).max())
    checked = undecided = 0
    rel = [1e-6, 1e-9, 1e-11, 1e-12, 1e-13, 1e-14]
    facs = [1.0 - r for r in rel] + [1.0 + r for r in rel]
    for it in range(40):
        b2, _, _ = pb(g, c2, L)
        b1, _, _ = pb(b2, c1, L)
        b0, x, q = pb(b1, start, L)
        se2 = ((b0 - start) ** 2).sum(1)
        sea = np.abs(np.sqrt(x) - L)
        c1, _, _ = pb(start, b1, L)
        c2, _, _ = pb(c1, b2, L)
        for k in range(0, len(se2), 97):
            ts = [se2[k] * f for f in facs] + [se2[k], np.nextafter(se2[k], 0),
                                               np.nextafter(se2[k], 1), sea[k] * sea[k]]
            for tol2 in ts:
                if not (tol2 > 0 and np.isfinite(tol2)):
                    continue
                lo, hi, _ = band(tol2, n1max, 4 * L)
                if sea[k] > hi:
                    assert se2[k] > tol2
                    checked += 1
                elif sea[k] < lo:
                    assert se2[k] <= tol2
                    checked += 1
                else:
                    undecided += 1
    assert checked > 5000 and undecided > 1000


def test_band_at_tol_zero_decides_nothing(plan_check):
    """tol = 0 (tol2 = 0): fabrik.py:57 stops only where both errors are exactly 0.
    A band with hi = 0 would call every lane with |1 - q| sqrt(x) > 0 "above tol",
    also one whose b0 rounds exactly onto start (se2 == 0) while q is an ulp off 1
    (not met on the trajectories below, where se2 == 0 comes with
    q == 1, but nothing rules it out).  fabrik_band returns (lo, hi) = (-1, inf)
    for tol2 <= 0 and NaN (asserted by the check program, and read off its --band lines
    here), so no lane is decided by it and every comparison is exact;
    tests/test_gpu_parity.py::test_fabrik_tol_zero_and_negative checks the kernels."""
    none = [r for r in plan_check if not r[0] > 0.0]  # tol2 in {0, -0.0, -1, -inf, NaN}
    assert len(none) >= 5 and any(math.isnan(r[0]) for r in none)
    assert {math.copysign(1.0, r[0]) for r in none if r[0] == 0.0} == {1.0, -1.0}
    for r in none:
        assert r[3] == -1.0 and r[4] == np.inf, "fabrik_band must decide nothing for tol2 <= 0"
    rng = np.random.default_rng(7)
    L = 2.0
    J, g = chains(4000, rng)
    g = J[0] + (g - J[0]) * 0.4  # mostly reachable goals, so chains converge
    start, c1, c2 = J[0], J[1], J[2]
    lo, hi, _ = band(0.0, 100.0, 8.0)
    assert lo < 0.0 and hi == np.inf
    zero = 0
    for _ in range(100):
        b2, _, _ = pb(g, c2, L)
        b1, _, _ = pb(b2, c1, L)
        b0, x, q = pb(b1, start, L)
        se2 = ((b0 - start) ** 2).sum(1)
        sea = np.abs(np.sqrt(x) - L)
        zero += int((se2 == 0.0).sum())
        # at tol2 = 0 the band never claims a decision
        assert not (sea > hi).any() and not (sea < lo).any()
        c1, _, _ = pb(start, b1, L)
        c2, _, _ = pb(c1, b2, L)
    assert zero > 0  # converged chains do reach se2 == 0, where tol 0 can stop


def test_quotient_domain_test_evidence(plan_check):
    """The iteration's core-domain test reads the quotients (ik_fabrik_step.h,
    fabrik_step4_lazy / fabrik_qmax, r06): |q1| + |q| + |q2| + |cq| <= min|L| 2^382.
    It is sound only if every radicand below sqrt_core's domain gives a quotient
    that is NaN or above |L| 2^382 on the hardware -- a property of v_rsq_f64 /
    v_rcp_f64 that no CPU can restate.  tools/dom_check.hip measured it on gfx950
    (2^30 radicands per link length over every binade below 2^-767, subnormals
    included, and 0 / inf / NaN); this pins the committed record and the source's
    threshold: the check program (plan_check) asserts fabrik_qmax == min |L| 2^382
    exactly, negative links and the minimum in every position included."""
    import json
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    import re
    # (the specials' quotients print as C's nan / -nan, not JSON: dropped, their verdict
    # is specials_flagged)
    rows = [json.loads(re.sub(r'"q\(0,inf,nan\)": \[[^\]]*\], ', "", l))
            for l in open(os.path.join(root, "profiles", "r06", "ab", "dom_check.json"))]
    assert len(rows) >= 5
    for r in rows:
        assert r["below_domain_passed"] == 0, r
        assert r["specials_flagged"] is True, r
        assert r["radicands"] >= 2 ** 30
    assert any(abs(r["L"]) < 2.0 ** -90 for r in rows) and any(abs(r["L"]) > 2.0 ** 90 for r in rows)
    src = open(os.path.join(root, "inversekinematicsann_amd", "csrc", "ik_fabrik_step.h")).read()
    assert "(fabs(q1) + fabs(q)) + (fabs(q2) + fabs(cq)) <= qmax" in src
