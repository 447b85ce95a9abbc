"""ANN inverse kinematics on the GPU -- kinematics/ann.py of the reference.

ANN.predict(positions) -> float32 (n, 4) exactly as the reference's
x-scaler -> Keras Sequential -> y-scaler pipeline (ann.py:70-76), computed by
libikhip's single fused kernel (fp32 MFMA layer chain, scalers in float64).

Model files (ann.py:78-95):
  * `<name>.h5` (Keras HDF5, read by models/keras_h5.py without h5py) with the
    reference's `<name>_scaler_x.bin` / `<name>_scaler_y.bin` beside it
    (decoded by models/scaler_bin.py without unpickling);
  * save_model() writes that same layout (`<prefix>_<timestamp>.h5` through
    models/hdf5_write.py, the scalers as joblib-dumped sklearn StandardScalers)
    so the reference's load_model can open it; `<name>.npz` (weights,
    activations and scalers) is also read.
Training (ann.py:27-68): ANN.fit() runs the reference's recipe -- 67/33 split,
StandardScalers fitted on the training part, Adam on MSE in batches of 32 with
per-epoch shuffling, early stopping on val_loss -- with the forward, backward and
Adam kernels of libikhip (ik_train.hip); the split, the scalers and the
early-stopping loop are kinematics/train.py.  fit(..., fk_weight=W) adds W times the
mean squared |FK(theta) - p| of the network's own angles to the loss
(ik_ann_train_set_loss).  train_model() itself still raises.
"""
from __future__ import annotations

import os
from dataclasses import dataclass, field
from datetime import datetime
from typing import List

import numpy as np

from .. import _native
from ..models.scaler_bin import ScalerParams, load_scaler


@dataclass
class DenseModel:
    """A Keras Sequential of Dense layers: h = act(h @ W + b)."""
    weights: List[np.ndarray]
    biases: List[np.ndarray]
    activations: List[str]
    name: str = "model"
    layer_names: List[str] = field(default_factory=list)

    @property
    def dims(self):
        return [self.weights[0].shape[0]] + [w.shape[1] for w in self.weights]

    def count_params(self):
        return int(sum(w.size + b.size for w, b in zip(self.weights, self.biases)))

    def flops_per_point(self):
        return int(sum(2 * w.shape[0] * w.shape[1] for w in self.weights))


def glorot_model(dims=(3,) + (500,) * 12 + (4,), seed=0, hidden_act="tanh") -> DenseModel:
    """Random-init model of the reference architecture (ann.py:46-56: Input(3),
    12 x Dense(500, tanh), Dense(4)) with Keras' default initialisers
    (glorot_uniform kernels, zero biases)."""
    rng = np.random.default_rng(seed)
    Ws, bs, acts = [], [], []
    for i in range(len(dims) - 1):
        lim = np.sqrt(6.0 / (dims[i] + dims[i + 1]))
        Ws.append(rng.uniform(-lim, lim, (dims[i], dims[i + 1])).astype(np.float32))
        bs.append(np.zeros(dims[i + 1], np.float32))
        acts.append(hidden_act if i < len(dims) - 2 else "linear")
    return DenseModel(Ws, bs, acts, name=f"glorot_seed{seed}")


# The scalers shipped with the reference model (models/*_scaler_{x,y}.bin),
# decoded by models/scaler_bin.py; used with synthetic weights for benches.
REFERENCE_X_SCALER = ScalerParams(
    mean=np.array([2.2073088909641334, 0.19405985835497927, 1.494994275926956]),
    scale=np.array([1.7144761363570307, 2.7973201512836416, 2.140079230865925]), var=None)
REFERENCE_Y_SCALER = ScalerParams(
    mean=np.array([0.052229169532186454, 0.9236331507819656, -1.3859332319838136,
                   -0.42092474514907724]),
    scale=np.array([0.8768847052996848, 0.6520665510519178, 1.0214536342625566,
                    0.4481255851377674]), var=None)


def load_npz_model(path):
    with np.load(path, allow_pickle=False) as z:
        nl = int(z["n_layers"])
        Ws = [z[f"W{i}"].astype(np.float32) for i in range(nl)]
        bs = [z[f"b{i}"].astype(np.float32) for i in range(nl)]
        acts = [str(a) for a in z["acts"]]
        xs = ScalerParams(mean=z["x_mean"], scale=z["x_scale"], var=None)
        ys = ScalerParams(mean=z["y_mean"], scale=z["y_scale"], var=None)
    return DenseModel(Ws, bs, acts, name=os.path.basename(path)), xs, ys


def save_npz_model(path, model: DenseModel, xs: ScalerParams, ys: ScalerParams):
    arrs = {f"W{i}": w for i, w in enumerate(model.weights)}
    arrs.update({f"b{i}": b for i, b in enumerate(model.biases)})
    np.savez(path, n_layers=np.int32(len(model.weights)),
             acts=np.array(model.activations, dtype="<U16"), x_mean=xs.mean, x_scale=xs.scale,
             y_mean=ys.mean, y_scale=ys.scale, **arrs)


def as_features(position) -> np.ndarray:
    """The n x 3 float64 batch ANN.predict scales (ann.py:73): a single point
    (3,) is one row; any other width fails like the reference's StandardScaler
    (sklearn's feature-count check), never by reinterpreting the numbers."""
    pts = np.asarray(position, dtype=np.float64)
    if pts.ndim == 1 and pts.shape[0] == 3:
        pts = pts.reshape(1, 3)
    if pts.ndim == 2 and pts.shape[0] == 0:
        return np.empty((0, 3), np.float64)
    if pts.ndim != 2:
        raise ValueError(f"Expected 2D array, got {pts.ndim}D array instead")
    if pts.shape[1] != 3:
        raise ValueError(f"X has {pts.shape[1]} features, but StandardScaler is expecting 3 "
                         "features as input.")
    return np.ascontiguousarray(pts)


class ANN:
    """ANN class implementing the neural-network IK approach (ann.py:18-25)."""

    def __init__(self, effector_workspace_limits, dh_matrix):
        self.effector_workspace_limits = effector_workspace_limits
        self.dh_matrix = dh_matrix
        self.model = None
        self.x_data_skaler = None
        self.y_data_skaler = None
        self._uploaded_to = None
        # the joint limits predict_refined honours (AnnInverseKinematics sets them):
        # None, or what Context.set_joint_limits takes
        self.joint_limits = None

    def train_model(self, epochs, samples, features):
        raise NotImplementedError("ANN training (kinematics/ann.py:27-68) is not part of the "
                                  "MI355X inference engine; train with the reference and load "
                                  "the saved .h5 with load_model()")

    def fit(self, epochs, samples, features, *, batch_size=32, learning_rate=1e-5, patience=12,
            hidden=(12, 500, "tanh"), seed=0, test_size=0.33, split_seed=42,
            verbose=False, mse_weight=1.0, fk_weight=0.0) -> dict:
        """Train the network on the GPU as the reference's train_model does
        (ann.py:27-68): train_test_split(test_size, random_state=split_seed),
        StandardScalers fitted on the training part (data cast to float32 after
        scaling), Input(d) -> hidden Dense layers -> Dense(n_out) from
        glorot_model(seed=seed), Adam(learning_rate) on MSE in batches of batch_size
        (the last one short), each epoch's order a permutation from
        np.random.default_rng(seed), EarlyStopping(val_loss, patience,
        restore_best_weights=True).

        Early stopping is `val_loss < best` with a wait counter against patience.
        The best epoch's weights are kept on the host and installed at the end
        whether or not training stopped early (Keras restores them only on an
        early stop; the last epoch's weights are installed only if no epoch's
        val_loss was ever finite).

        mse_weight / fk_weight: the loss is mse_weight * mse + fk_weight * fk
        (ik_ann_train_set_loss), fk the mean squared |FK(theta) - p| of the network's
        own angles in the scalers' units undone.  With fk_weight > 0 the samples must
        be positions (3 columns) and the features 4 joint angles, the chain is
        self.dh_matrix when that is a 4 x 4 table (it becomes the context's robot),
        else the context's robot, and 'loss' / 'val_loss', early stopping with them,
        are the weighted totals.

        Returns {'loss': [...], 'val_loss': [...], 'best_epoch', 'stopped_epoch'}
        (kinematics/train.py early_stopping_loop), with fk_weight > 0 also the
        per-epoch lists 'fk' and 'val_fk'.  Afterwards predict() and save_model()
        work as for a loaded model."""
        from . import train as T
        x = np.asarray(samples, dtype=np.float64)
        y = np.asarray(features, dtype=np.float64)
        if x.ndim != 2 or y.ndim != 2 or x.shape[0] != y.shape[0]:
            raise ValueError(f"samples {x.shape} / features {y.shape}: expected two 2D arrays "
                             "with the same number of rows")
        tr, te = T.split_indices(x.shape[0], test_size, split_seed)
        xs, ys = T.fit_scaler(x[tr]), T.fit_scaler(y[tr])
        x_tr = xs.transform(x[tr]).astype(np.float32)
        y_tr = ys.transform(y[tr]).astype(np.float32)
        x_te = xs.transform(x[te]).astype(np.float32)
        y_te = ys.transform(y[te]).astype(np.float32)
        dims, acts = [x.shape[1]], []
        for count, units, act in T.parse_hidden(hidden):
            dims += [units] * count
            acts += [act] * count
        dims.append(y.shape[1])
        acts.append("linear")
        model = glorot_model(tuple(dims), seed=seed)
        model.activations = acts
        perm = T.epoch_permutations(seed)
        ctx = _native.context()
        ctx.train_begin(model.weights, model.biases, acts,
                        max_batch=max(int(batch_size), min(4096, len(te))), lr=learning_rate)
        with_fk = float(fk_weight) > 0.0
        fks, val_fks = [], []

        def run_epoch(e):
            out = ctx.train_epoch(perm(len(tr)), int(batch_size))
            if with_fk:
                f, vf = ctx.train_fk()
                fks.append(f)
                val_fks.append(vf)
            return out
        try:
            if (float(mse_weight), float(fk_weight)) != (1.0, 0.0):
                if with_fk and np.shape(self.dh_matrix) == (4, 4):
                    ctx.set_robot(self.dh_matrix)
                ctx.train_set_loss(mse_weight, fk_weight, xs.effective(), ys.effective())
            ctx.train_data(x_tr, y_tr, x_te, y_te)
            hist, best = T.early_stopping_loop(
                epochs, patience, run_epoch, lambda: ctx.train_get("weights"), verbose)
            if with_fk:
                hist["fk"], hist["val_fk"] = fks, val_fks
            if best is None and hist["loss"]:
                best = ctx.train_get("weights")
        finally:
            ctx.train_end()
        if best is not None:
            model.weights, model.biases = list(best[0]), list(best[1])
        model.name = "sequential"
        self.set_model(model, xs, ys)
        return hist

    def set_model(self, model: DenseModel, x_scaler: ScalerParams, y_scaler: ScalerParams):
        """Install an in-memory model (e.g. glorot_model()) and its scalers."""
        self.model = model
        self.x_data_skaler = x_scaler
        self.y_data_skaler = y_scaler
        self._uploaded_to = None
        return self.model

    def _ctx(self):
        ctx = _native.context()
        if self.model is None:
            raise RuntimeError("no model loaded: call load_model() first")
        if self._uploaded_to is not ctx or getattr(ctx, "_ann_owner", None) is not self:
            xm, xs = self.x_data_skaler.effective()
            ym, ys = self.y_data_skaler.effective()
            ctx.ann_load(self.model.weights, self.model.biases, self.model.activations,
                         xm, xs, ym, ys)
            self._uploaded_to = ctx
            ctx._ann_owner = self
        # this object's joint limits or none: another object's never leak into its calls
        ctx.set_joint_limits(self.joint_limits)
        return ctx

    def predict(self, position):
        """Scale input, run the network, rescale output (ann.py:70-76); no limit check."""
        pts = as_features(position)
        ang, _, _ = self._ctx().ann_solve(pts, check_limits=False)
        return ang

    def predict_checked(self, pts):
        """predict + the workspace check of AnnInverseKinematics.ikine (one launch)."""
        ang, _, st = self._ctx().ann_solve(pts, check_limits=True)
        return ang, st

    def predict_with_fk_error(self, position):
        """(angles, |FK(angles) - p|_2 per point, stats) -- the cli.py:54-61 round trip."""
        pts = as_features(position)
        ang, err, st = self._ctx().ann_solve(pts, check_limits=False, want_fk_err=True)
        return ang, err, st

    def predict_refined(self, position, tol=1e-6, max_iter=20, damping=1e-3, check_limits=False,
                        want_seed_fk_err=False):
        """predict + the damped-least-squares refine of the network's angles in one
        library call (ik_ann_solve_refined): (angles n x 4 float64, iters, fk_err,
        stats); with want_seed_fk_err the network's own |FK - p| is appended."""
        pts = as_features(position)
        ang, it, err, serr, st = self._ctx().ann_solve_refined(
            pts, tol=tol, max_iter=max_iter, damping=damping, check_limits=check_limits,
            want_seed_fk_err=want_seed_fk_err)
        return (ang, it, err, st, serr) if want_seed_fk_err else (ang, it, err, st)

    def load_model(self, model_h5):
        """Load model from file (ann.py:78-85)."""
        if model_h5.endswith(".npz"):
            model, xs, ys = load_npz_model(model_h5)
        else:
            from ..models.keras_h5 import load_keras_dense_model
            model = load_keras_dense_model(model_h5)
            modelname = model_h5[:-3]
            xs = load_scaler(f'{modelname}_scaler_x.bin')
            ys = load_scaler(f'{modelname}_scaler_y.bin')
        self.set_model(model, xs, ys)
        return self.model

    def save_model(self, prefix='model'):
        """Save model to `<prefix>_<timestamp>.h5` plus `..._scaler_x.bin` /
        `..._scaler_y.bin` (ann.py:87-95); returns the .h5 path."""
        from ..models.keras_h5 import save_keras_dense_model
        from ..models.scaler_bin import save_scaler
        timestamp_str = str(datetime.timestamp(datetime.now())).replace('.', '-')
        base = f'{prefix}_{timestamp_str}'
        save_keras_dense_model(f'{base}.h5', self.model)
        save_scaler(f'{base}_scaler_x.bin', self.x_data_skaler)
        save_scaler(f'{base}_scaler_y.bin', self.y_data_skaler)
        return f'{base}.h5'
