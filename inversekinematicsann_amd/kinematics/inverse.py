"""Inverse kinematics API -- drop-in for the reference's kinematics/inverse.py.

Same class names, constructor signatures, defaults, return types and
exceptions as kinematics/inverse.py:18-155; the batch is solved on the GPU in
one call instead of a Python loop over points:

* FabrikInverseKinematics.ikine -> libikhip ik_fabrik_solve (float64, iteration
  counts bit-exact with the reference);
* AnnInverseKinematics.ikine    -> libikhip ik_ann_solve (fused fp32 MLP);
* AnalyticInverseKinematics.ikine (not in the reference) -> libikhip
  ik_analytic_solve (closed form with a chosen tool pitch and elbow branch).

Errors follow the reference's sequential semantics: the workspace check covers
every point first (inverse.py:117,153) and raises OutOfRobotReachException for
the first point outside; otherwise the lowest-index point whose solve raised
decides the exception (ZeroDivisionError / ValueError), as the reference's loop
would have stopped there.
"""
from __future__ import annotations

from abc import ABC, abstractmethod
from math import atan2

import numpy as np

from .. import _native
from ..robot.robot import OutOfRobotReachException
from .analytic import ELBOWS
from .ann import ANN, as_features as as_ann_points
from .forward import ForwardKinematics
from .refine import joint_limit_arrays
from .fabrik import Fabrik

_ERR_EXC = {
    _native.IK_E_ZERODIV: (ZeroDivisionError, 'float division by zero'),
    _native.IK_E_DOMAIN: (ValueError, 'math domain error'),
    _native.IK_E_ANGLE_RANGE: (OutOfRobotReachException,
                               'Forward Kinematics exception, robot joints angles limits are '
                               '(-2pi, 2pi)'),
}


def limits_array(workspace_limits) -> np.ndarray:
    """{'x': [lo, hi], ...} in dict order -> [lo0, hi0, lo1, hi1, lo2, hi2];
    axes the dict does not name are unbounded (zip() in inverse.py:31 stops)."""
    lim = np.array([-np.inf, np.inf] * 3, np.float64)
    for i, (_, v) in enumerate(list(workspace_limits.items())[:3]):
        lim[2 * i], lim[2 * i + 1] = float(v[0]), float(v[1])
    return lim


def as_points(dest_points) -> np.ndarray:
    """The n x 3 float64 batch of destination points.  Every point must be 3D,
    as the reference's Point (point.py:12-14) requires; a wrong width raises its
    ValueError instead of being reinterpreted as other points."""
    pts = np.asarray(dest_points, dtype=np.float64)
    if pts.ndim == 2 and pts.shape[0] == 0:
        return np.empty((0, 3), np.float64)
    if pts.ndim == 1 and pts.shape[0] == 0:
        return np.empty((0, 3), np.float64)
    if pts.ndim != 2 or pts.shape[1] != 3:
        bad = pts.shape[1:] if pts.ndim >= 2 else pts.shape
        raise ValueError(f'3D Point input shape should be (3,) not {tuple(bad)}')
    return np.ascontiguousarray(pts)


class InverseKinematics(ABC):
    """Inverse kinematics base (inverse.py:18-40)."""

    def __init__(self, dh_matrix, joints_distances, workspace_limits):
        self.dh_matrix = dh_matrix
        self.joints_distances = joints_distances
        self.workspace_limits = workspace_limits
        self.fkine = ForwardKinematics(self.dh_matrix)
        self.last_stats = None

    def _ctx(self):
        """The process context holding this object's robot: uploaded when it
        differs from what the context holds (Context.set_robot compares), so
        objects with different robots can interleave and repeated calls of one
        object upload nothing.  Its joint limits likewise: this object's, or none
        (only AnnInverseKinematics with refine has any)."""
        ctx = _native.context()
        ctx.set_robot(np.asarray(self.dh_matrix, np.float64),
                      np.asarray(self.joints_distances, np.float64),
                      limits_array(self.workspace_limits))
        ctx.set_joint_limits(getattr(self, "joint_limits", None))
        return ctx

    def _raise_out_of_reach(self, dest_points, idx):
        raise OutOfRobotReachException(
            f'Inverse Kinematics exception, point {dest_points[idx]} '
            'is out of manipulator reach area! '
            f'Limits: {self.workspace_limits}')

    def check_limits(self, dest_points):
        """Raise OutOfRobotReachException for the first point outside the
        (inclusive) workspace box (inverse.py:26-35), checked on the GPU."""
        pts = as_points(dest_points)
        st = self._ctx().check_limits(pts)
        if st.first_oob >= 0:
            self._raise_out_of_reach(dest_points, st.first_oob)

    @abstractmethod
    def ikine(self, dest_points):
        """Calculate inverse kinematics"""


class FabrikInverseKinematics(InverseKinematics):
    """Reaching inverse kinematics using the FABRIK method (inverse.py:45-139)."""

    def __init__(self, dh_matrix, joints_distances, workspace_limits,
                 max_err=0.001, max_iterations_num=100):
        super().__init__(dh_matrix, joints_distances, workspace_limits)
        self.fabrik = Fabrik(joints_distances, max_err, max_iterations_num)
        self.last_iterations = None

    def ikine(self, dest_points):
        """Joint angles [theta1..theta4] (float64) for every destination point."""
        pts = as_points(dest_points)
        if pts.shape[0] == 0:
            return []
        ang, iters, _, st = self._ctx().fabrik_solve(pts, self.fabrik.err_margin,
                                                     self.fabrik.max_iter_num)
        self.last_stats = st
        self.last_iterations = iters
        if st.first_oob >= 0:
            self._raise_out_of_reach(dest_points, st.first_oob)
        # inverse.py:125 writes each point's theta_1 into dh_matrix[0][0]; the
        # value left behind is the one of the last point processed.
        last = st.first_err if st.first_err >= 0 else pts.shape[0] - 1
        self.dh_matrix[0][0] = float(atan2(pts[last, 1], pts[last, 0]))
        if st.first_err >= 0:
            exc, msg = _ERR_EXC.get(st.first_err_code, (RuntimeError, 'ikine failed'))
            raise exc(msg)
        return ang.tolist()


class AnnInverseKinematics(InverseKinematics):
    """Reaching inverse kinematics using the ANN method (inverse.py:142-155)."""

    def __init__(self, dh_matrix, joints_distances, workspace_limits, refine=None,
                 joint_limits=None):
        """refine: None (the reference's behaviour: the network's float32 angles),
        True, or a dict with any of tol / max_iter / damping: ikine then returns the
        angles polished by the library's damped-least-squares refine (float64;
        defaults 1e-6 / 20 / 1e-3, kinematics/refine.py) and sets last_iterations,
        last_fk_err and last_seed_fk_err.

        joint_limits: four entries, each (lo, hi) in [-pi, pi] or None for a free
        joint; the refine then keeps every limited angle inside its interval
        (include/ikhip.h "Joint limits").  Only with refine: the bare network cannot
        honour them (ValueError)."""
        super().__init__(dh_matrix, joints_distances, workspace_limits)
        self.ann = ANN(workspace_limits, dh_matrix)
        if joint_limits is not None:
            if refine is None or refine is False:
                raise ValueError("joint_limits need refine: the network alone cannot honour "
                                 "them")
            if len(list(joint_limits)) != 4:
                raise ValueError("joint_limits: four entries, each (lo, hi) or None")
            joint_limits = joint_limit_arrays(list(joint_limits))
        self.joint_limits = self.ann.joint_limits = joint_limits
        if refine is None or refine is False:
            self.refine = None
        else:
            opts = {} if refine is True else dict(refine)
            unknown = set(opts) - {"tol", "max_iter", "damping"}
            if unknown:
                raise ValueError(f"refine: unknown options {sorted(unknown)}")
            self.refine = opts
        self.last_iterations = None
        self.last_fk_err = None
        self.last_seed_fk_err = None

    def load_model(self, model_name):
        """Load a model (.h5 + _scaler_{x,y}.bin, or .npz) onto the GPU."""
        self.ann.load_model(model_name)

    def ikine(self, dest_points):
        """Predicted joint angles (float32 values as Python floats); with refine,
        the polished float64 angles."""
        pts = as_ann_points(dest_points)
        if pts.shape[0] == 0:
            return []
        self._ctx()
        if self.refine is not None:
            ang, it, err, st, serr = self.ann.predict_refined(
                pts, check_limits=True, want_seed_fk_err=True, **self.refine)
            self.last_iterations, self.last_fk_err, self.last_seed_fk_err = it, err, serr
        else:
            ang, st = self.ann.predict_checked(pts)
        self.last_stats = st
        if st.first_oob >= 0:
            self._raise_out_of_reach(dest_points, st.first_oob)
        return ang.tolist()


class AnalyticInverseKinematics(InverseKinematics):
    """Closed-form inverse kinematics with a chosen tool pitch (theta2 + theta3 +
    theta4) and elbow branch, for a robot that is a yaw joint followed by a planar
    three-link chain (libikhip ik_analytic_solve, kinematics/analytic.py).  Not in the
    reference.  pitch: None (the tool points away from the shoulder), a scalar or one
    value per point; elbow "up" (theta3 <= 0) or "down"; nearest: a pitch at which
    the goal cannot be reached moves to the nearest one at which it can."""

    def __init__(self, dh_matrix, joints_distances, workspace_limits, pitch=None, elbow="up",
                 nearest=False):
        super().__init__(dh_matrix, joints_distances, workspace_limits)
        if elbow not in ELBOWS:
            raise ValueError(f"elbow: {elbow!r} is neither 'up' nor 'down'")
        self.pitch = pitch
        self.elbow = elbow
        self.nearest = bool(nearest)
        self.last_pitch = None
        self.last_fk_err = None

    def ikine(self, dest_points, pitch=None):
        """Joint angles [theta1..theta4] (float64) for every destination point; a
        pitch given here overrides the constructor's."""
        pts = as_points(dest_points)
        if pts.shape[0] == 0:
            return []
        want = self.pitch if pitch is None else pitch
        ang, used, err, st = self._ctx().analytic_solve(pts, want, ELBOWS[self.elbow],
                                                        self.nearest)
        self.last_stats, self.last_pitch, self.last_fk_err = st, used, err
        if st.first_oob >= 0:
            self._raise_out_of_reach(dest_points, st.first_oob)
        if st.first_err >= 0:
            i = st.first_err
            asked = 'None' if want is None else np.broadcast_to(
                np.asarray(want, np.float64), (pts.shape[0],))[i]
            raise OutOfRobotReachException(
                f'Inverse Kinematics exception, point {dest_points[i]} cannot be reached '
                f'with tool pitch {asked}')
        return ang.tolist()
