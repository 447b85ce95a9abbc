"""Host side of ANN.fit -- the parts of the reference's train_model
(kinematics/ann.py:27-68) that are not the network's arithmetic: sklearn's
train_test_split, StandardScaler.fit and Keras' EarlyStopping, restated with
numpy so that neither sklearn nor Keras is needed.
"""
from __future__ import annotations

import math
from typing import Callable, Dict, List, Optional, Tuple

import numpy as np

from ..models.scaler_bin import ScalerParams


def split_indices(n: int, test_size: float = 0.33, split_seed: int = 42
                  ) -> Tuple[np.ndarray, np.ndarray]:
    """(train, test) row indices as sklearn.model_selection.train_test_split(
    ..., test_size=test_size, random_state=split_seed) picks them (ann.py:29-30):
    ShuffleSplit's n_test = ceil(test_size * n), one RandomState permutation, the
    test rows first."""
    n = int(n)
    n_test = int(math.ceil(test_size * n))
    n_train = n - n_test
    if n_train < 1 or n_test < 0:
        raise ValueError(f"With n_samples={n} and test_size={test_size}, the resulting train "
                         "set will be empty.")
    perm = np.random.RandomState(split_seed).permutation(n)
    return perm[n_test:n_test + n_train], perm[:n_test]


def fit_scaler(a) -> ScalerParams:
    """StandardScaler().fit(a) (ann.py:32,35): float64 mean and population
    variance per column, scale = sqrt(var) with a zero-variance column's scale 1."""
    a = np.asarray(a, dtype=np.float64)
    if a.ndim != 2 or a.shape[0] < 1:
        raise ValueError(f"Expected a 2D array with at least one row, got shape {a.shape}")
    mean = a.mean(axis=0)
    var = a.var(axis=0)
    scale = np.sqrt(var)
    # sklearn's _handle_zeros_in_scale: a constant column keeps scale 1
    scale[scale < 10 * np.finfo(np.float64).eps] = 1.0
    return ScalerParams(mean=mean, scale=scale, var=var, n_samples_seen=int(a.shape[0]))


def early_stopping_loop(epochs: int, patience: int,
                        run_epoch: Callable[[int], Tuple[float, float]],
                        get_weights: Callable[[], object],
                        verbose: bool = False) -> Tuple[Dict, Optional[object]]:
    """Keras' fit loop under EarlyStopping(monitor='val_loss', patience=patience,
    restore_best_weights=True) (ann.py:58-68), over an injected stepper:
    run_epoch(e) trains epoch e (0-based) and returns (loss, val_loss);
    get_weights() snapshots the weights after it.

    An epoch improves when val_loss < best (a tie does not); otherwise a wait
    counter goes up and training stops once it reaches `patience`.  Returns
    (history, best_weights): history holds the per-epoch 'loss' / 'val_loss' lists,
    'best_epoch' (0-based, -1 if no epoch improved, e.g. every val_loss NaN) and
    'stopped_epoch' (0-based epoch training stopped at, 0 if it ran all epochs:
    Keras' convention).  best_weights is the best epoch's snapshot whether or not
    training stopped early -- Keras restores only on an early stop; here the best
    validation weights are what a caller always gets -- or None if none improved.
    """
    hist: Dict = {"loss": [], "val_loss": [], "best_epoch": -1, "stopped_epoch": 0}
    best = math.inf
    best_w = None
    wait = 0
    for e in range(int(epochs)):
        loss, val = run_epoch(e)
        hist["loss"].append(float(loss))
        hist["val_loss"].append(float(val))
        if verbose:
            print(f"Epoch {e + 1}/{epochs} - loss: {loss:.6g} - val_loss: {val:.6g}")
        if val < best:
            best = float(val)
            best_w = get_weights()
            hist["best_epoch"] = e
            wait = 0
        else:
            wait += 1
            if wait >= patience:
                hist["stopped_epoch"] = e
                break
    return hist, best_w


def epoch_permutations(seed: int):
    """Per-epoch shuffles: successive permutations of one default_rng(seed)."""
    rng = np.random.default_rng(seed)

    def perm(n: int) -> np.ndarray:
        return rng.permutation(n).astype(np.int32)
    return perm


def parse_hidden(hidden) -> List[Tuple[int, int, str]]:
    """hidden=(count, units, activation) or a list of such (ann.py:48-54 net_shape)."""
    if len(hidden) == 3 and isinstance(hidden[2], str):
        hidden = [hidden]
    return [(int(c), int(u), str(a)) for c, u, a in hidden]
