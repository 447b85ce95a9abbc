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


def fk_loss_reference(a, x, y, x_scaler, y_scaler, dh, mse_weight=1.0, fk_weight=0.0,
                      act="linear"):
    """The loss kernel's row arithmetic with the forward-kinematics term
    (csrc/ik_train_fk_row.h, ik_ann_train_set_loss) in numpy float64, on
    refine._chain / _consts.

    a: the last layer's outputs (rows x 4), x: the scaled inputs (rows x 3), y: the
    scaled labels (rows x 4); x_scaler / y_scaler: (mean, scale) pairs; dh: the 4 x 4
    DH table; act: the last layer's activation.  With theta = a y_scale + y_mean,
    p = x x_scale + x_mean and e = FK(wrap(theta)) - p (NaN when some |alpha_i| > 2 pi):

        mse_sum = sum (a - y)^2            the batch's mse is mse_sum / (rows 4)
        fk_sum  = sum e . e                the batch's fk  is fk_sum / rows
        dZ[r][j] = (mse_weight 2 (a_j - y_j) / (rows 4)
                    + fk_weight (2 / rows) (J_j . e) y_scale_j) act'(a_j)

    Returns (mse_sum, fk_sum, dZ rows x 4 float64)."""
    from .refine import _chain, _consts, wrap
    a = np.asarray(a, np.float64).reshape(-1, 4)
    x = np.asarray(x, np.float64).reshape(-1, 3)
    y = np.asarray(y, np.float64).reshape(-1, 4)
    xm, xs = (np.asarray(v, np.float64).reshape(3) for v in x_scaler)
    ym, ys = (np.asarray(v, np.float64).reshape(4) for v in y_scaler)
    rows = a.shape[0]
    consts = _consts(dh, np.float64)
    with np.errstate(all="ignore"):
        th = wrap(a * ys + ym)
        p = x * xs + xm
        (fx, fy, fz), cols = _chain(consts, th)
        e = np.stack([fx - p[:, 0], fy - p[:, 1], fz - p[:, 2]], axis=1)
        if consts[4]:
            e = np.full_like(e, np.nan)
        je = np.stack([c[0] * e[:, 0] + c[1] * e[:, 1] + c[2] * e[:, 2] for c in cols], axis=1)
        d = a - y
        deriv = {"linear": np.ones_like(a), "tanh": 1.0 - a * a,
                 "relu": (a > 0).astype(np.float64), "sigmoid": a * (1.0 - a)}[act]
        dz = (float(mse_weight) * 2.0 / (rows * 4.0) * d
              + float(fk_weight) * 2.0 / rows * je * ys) * deriv
        return float((d * d).sum()), float((e * e).sum()), dz


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
