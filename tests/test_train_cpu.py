"""CPU-only checks of the training feature's host side: the train/test split,
the scalers, the early-stopping loop (over a scripted stepper), and that the
header and the binding list carry the training calls."""
import math
import os
import re

import numpy as np
import pytest

from tests.conftest import ROOT

TRAIN_SYMBOLS = ["ik_ann_train_begin", "ik_ann_train_data", "ik_ann_train_grads",
                 "ik_ann_train_step", "ik_ann_train_epoch", "ik_ann_train_get",
                 "ik_ann_train_end"]


@pytest.mark.parametrize("n", [10, 100, 100000])
def test_split_matches_sklearn(n):
    ms = pytest.importorskip("sklearn.model_selection")
    from inversekinematicsann_amd.kinematics.train import split_indices
    tr, te = split_indices(n, 0.33, 42)
    rtr, rte = ms.train_test_split(np.arange(n), test_size=0.33, random_state=42)
    assert np.array_equal(tr, rtr) and np.array_equal(te, rte)
    if n == 100000:  # the n_samples_seen of the reference's shipped scaler
        assert (len(tr), len(te)) == (67000, 33000)


def test_split_sizes_without_sklearn():
    from inversekinematicsann_amd.kinematics.train import split_indices
    for n in (3, 10, 2048, 100000):
        tr, te = split_indices(n)
        assert len(te) == math.ceil(0.33 * n) and len(tr) + len(te) == n
        assert sorted(np.concatenate([tr, te]).tolist()) == list(range(n))


def test_fit_scaler_matches_sklearn():
    pp = pytest.importorskip("sklearn.preprocessing")
    from inversekinematicsann_amd.kinematics.train import fit_scaler
    rng = np.random.default_rng(4)
    a = rng.normal([2.0, -300.0, 1e-3, 7.0], [1.5, 40.0, 1e-5, 1.0], size=(5000, 4))
    a[:, 3] = 2.5  # zero variance
    ref = pp.StandardScaler().fit(a)
    sc = fit_scaler(a)
    for got, want in ((sc.mean, ref.mean_), (sc.var, ref.var_), (sc.scale, ref.scale_)):
        assert np.allclose(got, want, rtol=1e-12, atol=0.0)
    assert sc.scale[3] == 1.0
    assert sc.n_samples_seen == int(ref.n_samples_seen_) == 5000
    assert np.allclose(sc.transform(a), ref.transform(a), rtol=1e-12, atol=1e-12)


def test_fit_scaler_zero_variance_scale_is_one():
    from inversekinematicsann_amd.kinematics.train import fit_scaler
    a = np.column_stack([np.arange(10.0), np.full(10, 0.1), np.zeros(10)])
    sc = fit_scaler(a)
    assert sc.scale[1] == 1.0 and sc.scale[2] == 1.0
    assert sc.scale[0] == pytest.approx(np.sqrt(8.25), rel=1e-15)
    assert sc.mean[1] == pytest.approx(0.1, rel=1e-15)


def _scripted(vals):
    """A stepper whose weights after epoch e are [e]; loss = 10 + e."""
    state = {"e": -1}

    def run_epoch(e):
        state["e"] = e
        return 10.0 + e, vals[e]

    return run_epoch, lambda: [state["e"]], state


def test_early_stopping_patience_and_restore():
    from inversekinematicsann_amd.kinematics.train import early_stopping_loop
    vals = [5.0, 4.0, 4.5, 4.2, 4.1, 3.0, 9.0]
    run, get, state = _scripted(vals)
    hist, best = early_stopping_loop(len(vals), 3, run, get)
    # epoch 1 is the best; epochs 2, 3, 4 do not improve: stop at epoch 4 (patience 3)
    assert hist["val_loss"] == vals[:5] and hist["loss"] == [10.0, 11.0, 12.0, 13.0, 14.0]
    assert hist["best_epoch"] == 1 and hist["stopped_epoch"] == 4
    assert best == [1] and state["e"] == 4


def test_early_stopping_tie_is_no_improvement():
    from inversekinematicsann_amd.kinematics.train import early_stopping_loop
    vals = [2.0, 2.0, 2.0, 1.0]
    run, get, _ = _scripted(vals)
    hist, best = early_stopping_loop(4, 2, run, get)
    assert hist["best_epoch"] == 0 and hist["stopped_epoch"] == 2 and best == [0]
    assert len(hist["val_loss"]) == 3
    # with more patience the tie epochs only wait and the later improvement counts
    run, get, _ = _scripted(vals)
    hist, best = early_stopping_loop(4, 3, run, get)
    assert hist["best_epoch"] == 3 and hist["stopped_epoch"] == 0 and best == [3]


def test_early_stopping_runs_all_epochs_and_keeps_best():
    from inversekinematicsann_amd.kinematics.train import early_stopping_loop
    vals = [3.0, 1.0, 2.0, 1.5]
    run, get, state = _scripted(vals)
    hist, best = early_stopping_loop(4, 12, run, get)
    assert len(hist["loss"]) == 4 and hist["stopped_epoch"] == 0
    assert hist["best_epoch"] == 1 and best == [1] and state["e"] == 3
    # no finite val_loss: nothing improves, nothing to restore
    run, get, _ = _scripted([math.nan] * 3)
    hist, best = early_stopping_loop(3, 12, run, get)
    assert hist["best_epoch"] == -1 and best is None and len(hist["loss"]) == 3


def test_header_and_binding_list_have_training_calls():
    from inversekinematicsann_amd import _native
    with open(os.path.join(ROOT, "include", "ikhip.h")) as f:
        src = f.read()
    declared = set(re.findall(r"^\s*int\s+(ik_\w+)\s*\(", src, re.M))
    for sym in TRAIN_SYMBOLS:
        assert sym in declared, sym
        assert sym in _native.EXPORTED_SYMBOLS, sym
    lib = _native.load_library()
    for sym in TRAIN_SYMBOLS:
        assert hasattr(lib, sym), sym


def test_fit_exists_and_train_model_still_raises():
    from inversekinematicsann_amd.kinematics.ann import ANN
    assert callable(getattr(ANN, "fit"))
    with pytest.raises(NotImplementedError):
        ANN({}, []).train_model(1, [], [])


def test_fit_rejects_mismatched_rows():
    from inversekinematicsann_amd.kinematics.ann import ANN
    with pytest.raises(ValueError):
        ANN({}, []).fit(1, np.zeros((10, 3)), np.zeros((9, 4)))
