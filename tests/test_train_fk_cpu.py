"""The forward-kinematics loss term of training on the CPU: kinematics/train.py's
fk_loss_reference (the numpy float64 restatement of csrc/ik_train_fk_row.h) against
torch float64 autograd of an independently written chain (tests/train_fk_ref.py),
that every DH constant FK reads is live in it, and tests/host/train_fk_row_check.cpp,
which compiles the row header itself and the new plan functions."""
import os
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.robots import GEN_A, GEN_B, SIXDOF_DH, SKEW_DH, with_entry
from tests.train_fk_ref import X_SCALER, Y_SCALER, _torch, loss_parts

CLANGXX = "/opt/rocm/llvm/bin/clang++"  # csrc/Makefile HOSTCXX
CSRC = os.path.join(ROOT, "inversekinematicsann_amd", "csrc")
TABLES = {"SIXDOF_DH": SIXDOF_DH, "GEN_A": GEN_A, "GEN_B": GEN_B, "SKEW_DH": SKEW_DH}
# relative to the largest entry.  The two routes to FK agree to 1.3e-15 and to J^T e to
# 2.7e-15 (measured when the feature was specified); 1e-12 leaves room for the sums
# over 300 rows and is far below any wrong term.
BOUND = 1e-12


def _rows(rows, seed, shift=None):
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((rows, 4))
    x = rng.standard_normal((rows, 3)).astype(np.float32).astype(np.float64)
    y = rng.standard_normal((rows, 4)).astype(np.float32).astype(np.float64)
    if shift is not None:
        z = z * 0.1 + shift
    return z, x, y


def _autograd(z, x, y, dh, wm, wf, act, y_scaler=Y_SCALER):
    """(mse_sum, fk_sum, dLoss/dz, a) with a = act(z), by float64 autograd."""
    torch = _torch()
    zt = torch.tensor(z, dtype=torch.float64, requires_grad=True)
    a = torch.tanh(zt) if act == "tanh" else zt
    mse, fk = loss_parts(a, x, y, X_SCALER, y_scaler, dh)
    (wm * mse + wf * fk).backward()
    n = z.shape[0]
    return (float(mse.detach()) * n * 4, float(fk.detach()) * n, zt.grad.numpy(),
            a.detach().numpy())


def _rel(got, want):
    want = np.asarray(want, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - want).max() / np.abs(want).max())


@pytest.mark.parametrize("weights", [(0.0, 1.0), (1.0, 0.25), (1.0, 0.0)],
                         ids=["w0-1", "w1-0.25", "w1-0"])
@pytest.mark.parametrize("rows", [1, 24, 300])
@pytest.mark.parametrize("table", list(TABLES))
def test_reference_matches_float64_autograd(table, rows, weights):
    from inversekinematicsann_amd.kinematics.train import fk_loss_reference
    dh = TABLES[table]
    wm, wf = weights
    act = "tanh" if rows == 24 else "linear"
    z, x, y = _rows(rows, seed=rows)
    ms, fs, g, a = _autograd(z, x, y, dh, wm, wf, act)
    mse_sum, fk_sum, dz = fk_loss_reference(a, x, y, X_SCALER, Y_SCALER, dh, wm, wf, act=act)
    errs = (abs(mse_sum - ms) / ms, abs(fk_sum - fs) / fs, _rel(dz, g))
    print(f"{table} rows {rows} weights {weights}: mse {errs[0]:.2e}, fk {errs[1]:.2e}, "
          f"dZ {errs[2]:.2e}")
    assert max(errs) <= BOUND, errs
    assert dz.shape == (rows, 4) and dz.dtype == np.float64


def test_angles_beyond_two_pi_are_wrapped(monkeypatch):
    """theta between 2 pi and 3 pi (joints 1, 3) and below -2 pi (joints 2, 4): the same
    loss and gradient as autograd's, whose sines take any angle, and the chain is
    entered with wrapped angles only -- the device's sincos_fk is valid on
    [-2 pi, 2 pi] alone, so a restatement that left the wrap out would not be one."""
    from inversekinematicsann_amd.kinematics import refine
    from inversekinematicsann_amd.kinematics.train import fk_loss_reference
    seen = []
    chain = refine._chain

    def spy(consts, th):
        seen.append(np.array(th))
        return chain(consts, th)

    monkeypatch.setattr(refine, "_chain", spy)
    ym, ys = Y_SCALER
    shift = (np.array([7.8, -7.0, 8.4, -8.8]) - ym) / ys  # a = z: theta = shift's target + noise
    z, x, y = _rows(24, seed=5, shift=shift)
    raw = z * ys + ym
    assert ((raw[:, [0, 2]] > 2 * np.pi) & (raw[:, [0, 2]] < 3 * np.pi)).all()
    assert (raw[:, [1, 3]] < -2 * np.pi).all()
    for wm, wf in ((0.0, 1.0), (1.0, 0.25)):
        ms, fs, g, a = _autograd(z, x, y, SKEW_DH, wm, wf, "linear")
        mse_sum, fk_sum, dz = fk_loss_reference(a, x, y, X_SCALER, Y_SCALER, SKEW_DH, wm, wf)
        assert abs(mse_sum - ms) <= BOUND * ms and abs(fk_sum - fs) <= BOUND * fs
        assert _rel(dz, g) <= BOUND
    assert len(seen) == 2
    for th in seen:
        assert np.abs(th).max() <= np.pi * (1 + 1e-15)
        assert np.abs(np.remainder(th - raw + np.pi, 2 * np.pi) - np.pi).max() < 1e-13


def test_alpha_outside_range_gives_nan():
    from inversekinematicsann_amd.kinematics.train import fk_loss_reference
    z, x, y = _rows(5, seed=1)
    dh = with_entry(GEN_A, 3, 1, 7.0)  # |alpha_2| > 2 pi: FK raises in the reference
    mse_sum, fk_sum, dz = fk_loss_reference(z, x, y, X_SCALER, Y_SCALER, dh, 1.0, 0.25)
    assert np.isfinite(mse_sum) and np.isnan(fk_sum) and np.isnan(dz).all()


# (row, column) of d, a, alpha of the four joints in a DH table (rows theta, d, a, alpha)
ENTRIES = [(r, c) for r in (1, 2, 3) for c in range(4)]


@pytest.mark.parametrize("entry", ENTRIES, ids=[f"{'_daA'[r]}{c + 1}" for r, c in ENTRIES])
def test_every_constant_fk_reads_is_live(entry):
    """Changing one entry of GEN_A by 1e-3 moves dZ by more than 1e3 x BOUND, relative
    to its largest entry.  alpha_4 is the exception, and has to be: the effector is the
    translation of A_1 A_2 A_3 A_4 and A_4 = Rz Tz Tx Rx(alpha_4) ends in the rotation
    Rx(alpha_4), which turns the tool about its own origin and moves no position; the
    device never reads it either (RobotConstDev::jc[14..15] are unused by the chain).
    There the entry must change nothing at all, and autograd's chain, which does
    multiply by Rx(alpha_4), agrees."""
    from inversekinematicsann_amd.kinematics.train import fk_loss_reference
    z, x, y = _rows(24, seed=24)
    base = fk_loss_reference(z, x, y, X_SCALER, Y_SCALER, GEN_A, 0.0, 1.0)[2]
    dh = with_entry(GEN_A, *entry, GEN_A[entry] + 1e-3)
    moved = fk_loss_reference(z, x, y, X_SCALER, Y_SCALER, dh, 0.0, 1.0)[2]
    rel = _rel(moved, base)
    print(f"entry {entry}: dZ moves by {rel:.3e}")
    if entry == (3, 3):
        assert np.array_equal(moved, base)
        g = _autograd(z, x, y, dh, 0.0, 1.0, "linear")[2]
        assert _rel(moved, g) <= BOUND
    else:
        assert rel > 1e3 * BOUND


@pytest.mark.skipif(not os.path.exists(CLANGXX), reason="the ROCm clang++ is not installed")
def test_train_fk_row_check(tmp_path):
    exe = os.path.join(str(tmp_path), "train_fk_row_check")
    subprocess.run([CLANGXX, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", CSRC,
                    os.path.join(ROOT, "tests", "host", "train_fk_row_check.cpp"),
                    os.path.join(CSRC, "ik_train_plan.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-4000:]
    assert "train_fk_row_check ok" in r.stdout, r.stdout[-4000:]
