"""csrc/ik_chain_jac.h, the forward-kinematics chain with its Jacobian that the refine
kernel and the training loss's FK term both compile, in a stand-alone host program
(tests/host/chain_jac_check.cpp): byte for byte the numpy restatement
(kinematics/refine.py _chain_cs) when both are given the same sines and cosines, and
there against the long double matrix chain and the geometric Jacobian; csrc/ik_row.h's
wrap_pi beyond +-2 pi."""
import os
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.robots import GEN_A, GEN_B, SIXDOF_DH, SKEW_DH

CLANGXX = "/opt/rocm/llvm/bin/clang++"  # csrc/Makefile HOSTCXX
CSRC = os.path.join(ROOT, "inversekinematicsann_amd", "csrc")
TABLES = {"SIXDOF_DH": SIXDOF_DH, "GEN_A": GEN_A, "GEN_B": GEN_B, "SKEW_DH": SKEW_DH}
SPECIAL = (0.0, np.pi, -np.pi, np.pi / 2, -np.pi / 2)
N_RANDOM = 300


def angle_rows(seed):
    """N_RANDOM rows uniform in [-pi, pi], then rows with exactly 0, +-pi and +-pi/2:
    in every joint at once, in one joint beside random ones, and in all 625 mixtures."""
    rng = np.random.default_rng(seed)
    th = [rng.uniform(-np.pi, np.pi, (N_RANDOM, 4))]
    th.append(np.array([[v] * 4 for v in SPECIAL]))
    one = rng.uniform(-np.pi, np.pi, (len(SPECIAL) * 4, 4))
    for k, v in enumerate(SPECIAL):
        for j in range(4):
            one[4 * k + j, j] = v
    th.append(one)
    th.append(np.array(np.meshgrid(*[SPECIAL] * 4)).reshape(4, -1).T)
    return np.concatenate(th)


@pytest.mark.skipif(not os.path.exists(CLANGXX), reason="the ROCm clang++ is not installed")
def test_chain_header_in_host_program(tmp_path):
    from inversekinematicsann_amd.kinematics.refine import _chain, _chain_cs, _consts
    exe = os.path.join(str(tmp_path), "chain_jac_check")
    subprocess.run([CLANGXX, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", CSRC,
                    os.path.join(ROOT, "tests", "host", "chain_jac_check.cpp"), "-o", exe],
                   check=True)
    blocks, want = [np.array([float(len(TABLES))])], []
    for k, dh in enumerate(TABLES.values()):
        consts = _consts(dh, np.float64)
        a, d, ca, sa, alpha_bad = consts
        assert not alpha_bad
        th = angle_rows(11 + k)
        s, c = np.sin(th), np.cos(th)
        jc = np.stack([a, d, ca, sa], axis=1)  # fk_trip_consts: per joint a, d, cos, sin
        blocks += [np.array([float(len(th))]), np.asarray(dh, np.float64).ravel(), jc.ravel(),
                   np.concatenate([th, s, c], axis=1).ravel()]
        (x, y, z), J = _chain_cs(consts, s, c)
        want.append(np.stack([x, y, z, J[0][0], J[0][1], *J[1], *J[2], *J[3]], axis=1))
        # _chain is _chain_cs on numpy's sines and cosines
        (x1, y1, z1), J1 = _chain(consts, th)
        assert all(np.array_equal(p, q) for p, q in zip((x, y, z), (x1, y1, z1)))
        assert all(np.array_equal(p, q) for cp, cq in zip(J, J1) for p, q in zip(cp, cq))
        assert not J[0][2].any()  # column 1 has no z part
    want = np.concatenate(want)
    assert len(want) == len(TABLES) * (N_RANDOM + 5 + 20 + 625)
    rows, out = tmp_path / "rows.f64", tmp_path / "out.f64"
    np.concatenate(blocks).astype("<f8").tofile(rows)
    r = subprocess.run([exe, str(rows), str(out)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-4000:]
    assert "chain_jac_check ok" in r.stdout and f"rows {len(want)}:" in r.stdout, r.stdout[-4000:]
    got = np.fromfile(out, "<f8").reshape(-1, 14)
    assert got.shape == want.shape
    differ = np.flatnonzero((got.view(np.uint64) != want.view(np.uint64)).any(axis=1))
    assert got.tobytes() == want.astype("<f8").tobytes(), (differ[:10], got[differ[:3]],
                                                          want[differ[:3]])
