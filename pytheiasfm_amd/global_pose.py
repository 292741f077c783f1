"""Host-side mirror of pyTheia's global rotation estimation (pytheia.sfm.RobustRotationEstimator,
src/pytheia/sfm/sfm.cc:1749-1780 -> global_pose_estimation/robust_rotation_estimator.{h,cc}).

The solve runs on the device through theia_hip_robust_rotation_averaging (csrc/rotation_averaging.hip).  The object
keeps the reference's state across calls: constraints accumulate over EstimateRotations / AddRelativeRotationConstraint
calls on one object, and the view fixed by default on the first call stays fixed on later ones.
"""
import enum
import math

import numpy as np

from . import _capi as capi


class GlobalRotationEstimatorType(enum.IntEnum):  # reconstruction_estimator_options.h:64-70
    ROBUST_L1L2 = 0
    NONLINEAR = 1
    LINEAR = 2
    LAGRANGE_DUAL = 3
    HYBRID = 4


class RobustRotationEstimatorOptions:  # robust_rotation_estimator.h:64-84
    def __init__(self):
        self.max_num_l1_iterations = 5
        self.l1_step_convergence_threshold = 0.001
        self.max_num_irls_iterations = 100
        self.irls_step_convergence_threshold = 0.001
        self.irls_loss_parameter_sigma = math.radians(5.0)

    def to_c(self):
        o = capi.RotationOptions()
        o.max_num_l1_iterations = int(self.max_num_l1_iterations)
        o.max_num_irls_iterations = int(self.max_num_irls_iterations)
        o.l1_step_convergence_threshold = float(self.l1_step_convergence_threshold)
        o.irls_step_convergence_threshold = float(self.irls_step_convergence_threshold)
        o.irls_loss_parameter_sigma = float(self.irls_loss_parameter_sigma)
        return o


def robust_rotation_averaging(orientations, edges, relative_rotations, fixed=None, options=None):
    """The C-ABI on arrays: orientations [n][3] (not modified), edges [E][2] view indices, relative_rotations [E][3],
    fixed: [n] booleans or None.  Returns (return code, new orientations [n][3], RotationSummary); the orientations are
    those the call left behind (the input on INVALID_ARGUMENT, the state reached so far on ERR_INTERNAL)."""
    o = (options or RobustRotationEstimatorOptions()).to_c()
    aa = np.array(orientations, dtype=np.float64).reshape(-1, 3)
    e = np.ascontiguousarray(np.asarray(edges, dtype=np.int32).reshape(-1, 2))
    r = np.ascontiguousarray(np.asarray(relative_rotations, dtype=np.float64).reshape(-1, 3))
    f = None if fixed is None else np.ascontiguousarray(np.asarray(fixed, dtype=bool).astype(np.uint8))
    if f is not None and f.shape != (aa.shape[0],):
        raise ValueError("fixed must have one entry per view")
    if r.shape[0] != e.shape[0]:
        raise ValueError("one relative rotation per edge")
    s = capi.RotationSummary()
    rc = capi.lib().theia_hip_robust_rotation_averaging(aa.shape[0], capi.ptr(aa, capi.C.c_double), capi.ptr(f, capi.C.c_uint8),
                                                        e.shape[0], capi.ptr(e, capi.C.c_int32), capi.ptr(r, capi.C.c_double),
                                                        capi.C.byref(o), capi.C.byref(s))
    return rc, aa, s


class RobustRotationEstimator:
    """RobustRotationEstimator(options) with EstimateRotations(view_pairs, orientations) -> dict, as pyTheia binds it
    (EstimateRotationsWrapper: the dict comes back whether the solve succeeded or not)."""

    def __init__(self, options):
        self.options = options
        self._constraints = []      # [((id1, id2), aa)] in the order they were added
        self._fixed = set()
        self.last_summary = None
        self.last_success = None

    def AddRelativeRotationConstraint(self, view_id_pair, relative_rotation):
        self._constraints.append(((int(view_id_pair[0]), int(view_id_pair[1])),
                                  np.asarray(relative_rotation, dtype=np.float64).reshape(3).copy()))

    def SetFixedGlobalRotations(self, fixed_views):
        self._fixed = {int(v) for v in fixed_views}

    def EstimateRotations(self, view_pairs, orientations):
        for pair, info in view_pairs.items():
            self.AddRelativeRotationConstraint(pair, info.rotation_2)
        return self._estimate(orientations)

    def _estimate(self, orientations):
        ids = [int(k) for k in orientations]
        if not self._constraints:   # CHECK_GT(relative_rotations_.size(), 0)
            raise capi.TheiaHipError(capi.THEIA_HIP_ERR_INVALID_ARGUMENT, "no relative rotation constraints")
        if not ids:
            raise capi.TheiaHipError(capi.THEIA_HIP_ERR_INVALID_ARGUMENT, "no orientations")
        if not self._fixed:
            self._fixed = {ids[0]}  # the reference fixes begin(*global_orientations) and keeps it
        pos = {v: k for k, v in enumerate(ids)}
        missing = sorted(v for v in self._fixed if v not in pos)
        if missing:                 # the reference sizes A by the fixed-set size: a CHECK-class failure
            raise capi.TheiaHipError(capi.THEIA_HIP_ERR_INVALID_ARGUMENT, f"fixed view {missing[0]} has no orientation")
        try:
            edges = np.array([(pos[a], pos[b]) for (a, b), _ in self._constraints], dtype=np.int32)
        except KeyError as ex:      # FindOrDie
            raise capi.TheiaHipError(capi.THEIA_HIP_ERR_INVALID_ARGUMENT, f"view {ex.args[0]} has no orientation") from None
        rel = np.array([r for _, r in self._constraints], dtype=np.float64)
        aa = np.array([np.asarray(orientations[v], dtype=np.float64).reshape(3) for v in ids])
        fixed = np.array([v in self._fixed for v in ids])
        rc, out, s = robust_rotation_averaging(aa, edges, rel, fixed, self.options)
        if rc not in (0, capi.THEIA_HIP_ERR_INTERNAL):
            capi.check(rc)
        self.last_success = rc == 0
        self.last_summary = s
        return {v: out[k].copy() for k, v in enumerate(ids)}
