"""Host-side mirror of pyTheia's global rotation estimation (pytheia.sfm.RobustRotationEstimator,
src/pytheia/sfm/sfm.cc:1749-1780 -> global_pose_estimation/robust_rotation_estimator.{h,cc}) and position estimation
(pytheia.sfm.LeastUnsquaredDeviationPositionEstimator, sfm.cc:1707-1726 ->
global_pose_estimation/least_unsquared_deviation_position_estimator.{h,cc}).

The solve runs on the device through theia_hip_robust_rotation_averaging (csrc/rotation_averaging.hip).  The object
keeps the reference's state across calls: constraints accumulate over EstimateRotations / AddRelativeRotationConstraint
calls on one object, and the view fixed by default on the first call stays fixed on later ones.  The estimator that
needs no initial guess, pytheia.sfm.LinearRotationEstimator (sfm.cc:1789-1795 ->
global_pose_estimation/linear_rotation_estimator.{h,cc}), runs through theia_hip_linear_rotations
(csrc/linear_rotations.hip); the Ceres refinement of given orientations, pytheia.sfm.NonlinearRotationEstimator
(sfm.cc:1782-1787 -> global_pose_estimation/nonlinear_rotation_estimator.{h,cc}), through theia_hip_nonlinear_rotations
(csrc/nonlinear_rotations.hip); both pipelines seed it with OrientationsFromMaximumSpanningTree
(view_graph/orientations_from_maximum_spanning_tree.cc), host code here as there.  The two estimators that certify their
answer, pytheia.sfm.LagrangeDualRotationEstimator and HybridRotationEstimator (sfm.cc:1797-1807 ->
global_pose_estimation/lagrange_dual_rotation_estimator.{h,cc}, hybrid_rotation_estimator.{h,cc}), run through
theia_hip_lagrange_dual_rotations (csrc/lagrange_dual_rotations.hip), the second followed by the IRLS half of
theia_hip_robust_rotation_averaging.  The positions run
through theia_hip_lud_positions (csrc/lud_positions.hip), or, from the tracks' features and without the pairs' relative
translations, through theia_hip_ligt_positions (pytheia.sfm.LiGTPositionEstimator, sfm.cc:1728-1747 ->
global_pose_estimation/LiGT_position_estimator.{h,cc}; csrc/ligt_positions.hip), or, from the pairs' relative poses and
the features together, through theia_hip_linear_triplet_positions (pytheia.sfm.LinearPositionEstimator ->
global_pose_estimation/linear_position_estimator.{h,cc}; csrc/linear_positions.hip), or, by the Ceres solve over the
pairs' rotated translations and the rays of a few selected tracks, through theia_hip_nonlinear_positions
(NonlinearPositionEstimator -> global_pose_estimation/nonlinear_position_estimator.{h,cc}, the reference's default
position stage; csrc/nonlinear_positions.hip).

Between them sit the two view-graph filters (sfm/filter_view_pairs_from_orientation.{h,cc} after the rotations,
sfm/filter_view_pairs_from_relative_translation.{h,cc}, the 1DSfM test, before the positions): csrc/view_pair_filters.hip
behind filter_pairs_from_orientation / filter_translations_1dsfm on arrays and FilterViewPairsFromOrientation /
FilterViewPairsFromRelativeTranslation on the {(id1, id2): TwoViewInfo} dict that stands in for the ViewGraph.
The two prunings that need no orientations (sfm/filter_view_graph_cycles_by_rotation.{h,cc} before the first rotation
stage, sfm/view_graph/remove_disconnected_view_pairs.{h,cc} after every filter) are csrc/view_graph_pruning.hip behind
filter_cycles_by_rotation / remove_disconnected_pairs on arrays and FilterViewGraphCyclesByRotation /
RemoveDisconnectedViewPairs on the dict.
"""
import ctypes as C
import enum
import math

import numpy as np

from . import _capi as capi
from .synth import angle_axis_to_matrix


class GlobalRotationEstimatorType(enum.IntEnum):  # reconstruction_estimator_options.h:64-70
    # on the device: ROBUST_L1L2 (RobustRotationEstimator), NONLINEAR (NonlinearRotationEstimator), LINEAR
    # (LinearRotationEstimator), LAGRANGE_DUAL (LagrangeDualRotationEstimator: the rank-restricted SDP relaxation by block
    # coordinate minimisation with the Riemannian staircase) and HYBRID (HybridRotationEstimator: that, then IRLS)
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


class LinearRotationEstimatorOptions:
    """The two stopping rules of the block inverse iteration (the reference's class has no options: it hands Spectra 1000
    iterations and a tolerance of 1e-4, linear_rotation_estimator.cc:178)."""

    def __init__(self):
        self.max_num_iterations = 1000
        self.subspace_convergence_threshold = 1e-10

    def to_c(self):
        o = capi.LinearRotationOptions()
        o.max_num_iterations = int(self.max_num_iterations)
        o.subspace_convergence_threshold = float(self.subspace_convergence_threshold)
        return o


def linear_rotations(num_views, edges, relative_rotations, options=None, orientations_out=None):
    """theia_hip_linear_rotations on arrays: edges [E][2] view indices, relative_rotations [E][3] = TwoViewInfo::rotation_2.
    Returns (return code, orientations [num_views][3], estimated [num_views] bool, LinearRotationSummary); a view without
    an edge keeps its orientations_out row (zeros without orientations_out); on a refusal nothing is written.  The
    orientations are defined up to one common rotation on the right."""
    o = (options or LinearRotationEstimatorOptions()).to_c()
    n = int(num_views)
    e, r = _pair_arrays(edges, relative_rotations, "relative rotation")
    out = np.zeros((max(n, 0), 3)) if orientations_out is None else orientations_out
    if out.shape != (n, 3) or out.dtype != np.float64 or not out.flags["C_CONTIGUOUS"]:
        raise ValueError("orientations_out must be a C-contiguous float64 [num_views][3] array")
    est = np.zeros(max(n, 0), dtype=np.uint8)
    s = capi.LinearRotationSummary()
    rc = capi.lib().theia_hip_linear_rotations(n, e.shape[0], capi.ptr(e, C.c_int32), capi.ptr(r, C.c_double), C.byref(o),
                                               capi.ptr(out, C.c_double), capi.ptr(est, C.c_uint8), C.byref(s))
    return rc, out, est.astype(bool), s


class LinearRotationEstimator:
    """LinearRotationEstimator() with AddRelativeRotationConstraint(view_id_pair, relative_rotation) and
    EstimateRotations(view_pairs, orientations=None) -> dict (sfm.cc:1789-1795 -> linear_rotation_estimator.{h,cc}).

    The views are indexed in the order the constraints first name them (InsertIfNotPresent, :97-98), and the constraints
    accumulate over the calls on one object (constraint_entries_ is a member).  A view id already in `orientations` keeps
    the value passed in (the reference's emplace does not overwrite, :200); the dict returned holds those entries and
    every view of the constraints.  pyTheia's binding returns only the bool, and its dict argument is a copy the caller
    never sees: this mirror returns the dict, as RobustRotationEstimator's binding does, and keeps the bool in
    last_success."""

    def __init__(self):
        self._constraints = []      # [((id1, id2), aa)] in the order they were added
        self.last_summary = None
        self.last_success = None

    def AddRelativeRotationConstraint(self, view_id_pair, relative_rotation):
        self._constraints.append(((int(view_id_pair[0]), int(view_id_pair[1])),
                                  np.asarray(relative_rotation, dtype=np.float64).reshape(3).copy()))

    def EstimateRotations(self, view_pairs, orientations=None):
        for pair, info in view_pairs.items():
            self.AddRelativeRotationConstraint(pair, info.rotation_2)
        if not self._constraints:   # CHECK_GT(constraint_entries_.size(), 0)
            raise capi.TheiaHipError(capi.THEIA_HIP_ERR_INVALID_ARGUMENT, "no relative rotation constraints")
        ids = {}
        for (a, b), _ in self._constraints:
            ids.setdefault(a, len(ids))
            ids.setdefault(b, len(ids))
        edges = np.array([(ids[a], ids[b]) for (a, b), _ in self._constraints], dtype=np.int32)
        rel = np.array([r for _, r in self._constraints], dtype=np.float64)
        rc, out, _, s = linear_rotations(len(ids), edges, rel)
        if rc not in (0, capi.THEIA_HIP_ERR_INTERNAL):
            capi.check(rc)
        self.last_success = rc == 0
        self.last_summary = s
        result = {} if orientations is None else {int(v): np.asarray(r, dtype=np.float64).reshape(3).copy()
                                                  for v, r in orientations.items()}
        for v, k in ids.items():
            result.setdefault(v, out[k].copy())
        return result


class SDPSolverType(enum.IntEnum):  # math/solver_options.h:43-49
    RBR_BCM = 0
    RANK_DEFICIENT_BCM = 1
    RIEMANNIAN_STAIRCASE = 2
    SE_SYNC = 3   # not implemented in the reference either
    SHONAN = 4    # not implemented in the reference either


class PreconditionerType(enum.IntEnum):  # math/solver_options.h:51-56; only None is implemented in the reference
    NONE = 0
    JACOBI = 1
    INCOMPLETE_CHOLESKY = 2
    REGULARIZED_CHOLESKY = 3


class SweepOrder(enum.IntEnum):
    """The order of a BCM sweep: INDEX is the reference's; COLOURED orders the views by (greedy colour, index), the
    reference's sweep on a relabelled graph, in as many launches per sweep as there are colours."""
    INDEX = 0
    COLOURED = 1


class RiemannianStaircaseOptions:  # math/solver_options.h:58-73
    def __init__(self):
        self.min_rank = 3
        self.max_rank = 10
        self.max_eigen_solver_iterations = 20   # of the reference's Lanczos; the certificate here is a factorisation
        self.min_eigenvalue_nonnegativity_tolerance = 1e-5
        self.num_Lanczos_vectors = 20           # likewise unused
        self.local_solver_type = SDPSolverType.RANK_DEFICIENT_BCM
        self.gradient_tolerance = 1e-2
        self.preconditioned_gradient_tolerance = 1e-4


class SDPSolverOptions:  # math/solver_options.h:75-97
    def __init__(self, max_iter=500, tol=1e-8, log=True):
        self.max_iterations = max_iter
        self.tolerance = tol
        self.verbose = log
        self.num_threads = 8
        self.solver_type = SDPSolverType.RIEMANNIAN_STAIRCASE
        self.preconditioner_type = PreconditionerType.NONE
        self.riemannian_staircase_options = RiemannianStaircaseOptions()
        self.sweep_order = SweepOrder.INDEX     # no counterpart in the reference

    def to_c(self):
        r = self.riemannian_staircase_options
        o = capi.LagrangeDualOptions()
        o.solver_type = int(self.solver_type)
        o.max_iterations = int(self.max_iterations)
        o.min_rank = int(r.min_rank)
        o.max_rank = int(r.max_rank)
        o.sweep_order = int(self.sweep_order)
        o.tolerance = float(self.tolerance)
        o.min_eigenvalue_nonnegativity_tolerance = float(r.min_eigenvalue_nonnegativity_tolerance)
        o.gradient_tolerance = float(r.gradient_tolerance)
        o.preconditioned_gradient_tolerance = float(r.preconditioned_gradient_tolerance)
        return o


LAGRANGE_DUAL_END_STATES = ("bcm", "certified", "max_rank", "escape_failed")   # THEIA_LAGRANGE_DUAL_END_*


def lagrange_dual_rotations(num_views, edges, relative_rotations, options=None, y_init=None, orientations_out=None,
                            want_y=False, want_log=False):
    """theia_hip_lagrange_dual_rotations on arrays: edges [E][2] view indices, relative_rotations [E][3] =
    TwoViewInfo::rotation_2, y_init: None or [rank][3 m] over the m views that have an edge, in view order.  Returns
    (return code, orientations [num_views][3], estimated [num_views] bool, LagrangeDualSummary) and then, with want_y,
    Y [final_rank][3 m] and, with want_log, the per-level log [levels][8] = (rank, sweeps, f, certified, lambda_min
    estimate, v' S v of the escape direction, accepted alpha, fallback used).  A view without an edge keeps its
    orientations_out row (zeros without orientations_out); on a refusal nothing is written."""
    o = (options or SDPSolverOptions()).to_c()
    n = int(num_views)
    e, r = _pair_arrays(edges, relative_rotations, "relative rotation")
    out = np.zeros((max(n, 0), 3)) if orientations_out is None else orientations_out
    if out.shape != (n, 3) or out.dtype != np.float64 or not out.flags["C_CONTIGUOUS"]:
        raise ValueError("orientations_out must be a C-contiguous float64 [num_views][3] array")
    est = np.zeros(max(n, 0), dtype=np.uint8)
    y0, rank_init = None, 0
    if y_init is not None:
        y0 = np.ascontiguousarray(np.asarray(y_init, dtype=np.float64))
        if y0.ndim != 2 or y0.shape[1] % 3:
            raise ValueError("y_init must be [rank][3 m]")
        in_range = e[(e >= 0).all(axis=1) & (e < n).all(axis=1)]
        if y0.shape[1] != 3 * len(np.unique(in_range)):
            raise ValueError("y_init must have three columns per view that has an edge")
        rank_init = y0.shape[0]
    cols = 3 * max(n, 1)
    y = np.zeros((12, cols)) if want_y else None
    log = np.full((16, 8), np.nan) if want_log else None
    s = capi.LagrangeDualSummary()
    rc = capi.lib().theia_hip_lagrange_dual_rotations(
        n, e.shape[0], capi.ptr(e, C.c_int32), capi.ptr(r, C.c_double), C.byref(o), rank_init, capi.ptr(y0, C.c_double),
        capi.ptr(out, C.c_double), capi.ptr(est, C.c_uint8), capi.ptr(y, C.c_double), C.byref(s), capi.ptr(log, C.c_double),
        16 if want_log else 0)
    ret = [rc, out, est.astype(bool), s]
    if want_y:   # the call wrote [final_rank][3 m] densely at the front of the buffer
        m3 = 3 * s.num_views_in_system
        ret.append(y.reshape(-1)[:s.final_rank * m3].reshape(s.final_rank, m3).copy())
    if want_log:
        ret.append(log[:min(s.num_levels, 16)].copy())
    return tuple(ret)


class LagrangeDualRotationEstimator:
    """LagrangeDualRotationEstimator(options=SDPSolverOptions()) with SetRAOption(options), GetRASummary() and
    EstimateRotations(view_pairs, orientations) -> dict (sfm.cc:1797-1801 -> lagrange_dual_rotation_estimator.{h,cc}), in
    NonlinearRotationEstimator's conventions: the input dict is not modified and the dict comes back whatever the
    staircase's end, the reference's bool (always true) is in last_success.

    `orientations` names the views (its values are not read: the estimator needs no initial guess); they are indexed in
    ascending id (ViewIdToAscentIndex).  A pair that names a view without an entry is refused (the reference's
    operator[] would give it index 0 silently).  A view without a pair keeps the value passed in.  The view whose
    orientation comes out as the identity is the lowest id that has a pair.  ComputeErrorBound / GetErrorBound are not
    part of EstimateRotations and are not built."""

    def __init__(self, options=None):
        self.options = options or SDPSolverOptions()
        self.last_summary = None
        self.last_success = None
        self.gauge_view = None

    def SetRAOption(self, options):
        self.options = options

    def GetRASummary(self):
        return self.last_summary

    def EstimateRotations(self, view_pairs, orientations):
        result = {int(v): np.asarray(r, dtype=np.float64).reshape(3).copy() for v, r in orientations.items()}
        ids = sorted(result)
        if not view_pairs:   # CHECK_GT(view_pairs.size(), 0)
            raise capi.TheiaHipError(capi.THEIA_HIP_ERR_INVALID_ARGUMENT, "no relative rotation constraints")
        if not ids:          # CHECK_GT(N, 0)
            raise capi.TheiaHipError(capi.THEIA_HIP_ERR_INVALID_ARGUMENT, "no orientations")
        pos = {v: k for k, v in enumerate(ids)}
        try:
            edges = np.array([(pos[int(a)], pos[int(b)]) for (a, b) in view_pairs], dtype=np.int32)
        except KeyError as ex:
            raise capi.TheiaHipError(capi.THEIA_HIP_ERR_INVALID_ARGUMENT, f"view {ex.args[0]} has no orientation") from None
        rel = np.array([np.asarray(info.rotation_2, dtype=np.float64).reshape(3) for info in view_pairs.values()])
        out = np.array([result[v] for v in ids])
        rc, out, est, s = lagrange_dual_rotations(len(ids), edges, rel, self.options, orientations_out=out)
        capi.check(rc)
        self.last_success = True
        self.last_summary = s
        self.gauge_view = ids[s.gauge_view]
        self._edges, self._rel, self._ids = edges, rel, ids
        return {v: out[k].copy() for k, v in enumerate(ids)}


class IRLSRefinerOptions:  # irls_rotation_local_refiner.h:54-66
    def __init__(self):
        self.num_threads = 8
        self.max_num_irls_iterations = 10
        self.irls_step_convergence_threshold = 0.001
        self.irls_loss_parameter_sigma = math.radians(5.0)


class HybridRotationEstimatorOptions:  # hybrid_rotation_estimator.h:53-56
    def __init__(self):
        self.sdp_solver_options = SDPSolverOptions()
        self.irls_options = IRLSRefinerOptions()


class HybridRotationEstimator:
    """HybridRotationEstimator(options=HybridRotationEstimatorOptions()) with EstimateRotations(view_pairs, orientations)
    -> dict (sfm.cc:1803-1807 -> hybrid_rotation_estimator.cc:69-109): LagrangeDualRotationEstimator, then the IRLS of
    irls_rotation_local_refiner.cc:77-160 alone -- theia_hip_robust_rotation_averaging with max_num_l1_iterations = 0 --
    from its result, with the gauge view held (the reference holds its view of index 0, which is the same view when that
    one has a pair).  last_success is the IRLS solve's outcome; last_summary the SDP stage's, last_irls_summary the
    refinement's."""

    def __init__(self, options=None):
        self.options = options or HybridRotationEstimatorOptions()
        self._ld = LagrangeDualRotationEstimator(self.options.sdp_solver_options)
        self.last_summary = None
        self.last_irls_summary = None
        self.last_success = None

    def EstimateRotations(self, view_pairs, orientations):
        self._ld.SetRAOption(self.options.sdp_solver_options)
        result = self._ld.EstimateRotations(view_pairs, orientations)
        self.last_summary = self._ld.last_summary
        ids, edges, rel = self._ld._ids, self._ld._edges, self._ld._rel
        io = self.options.irls_options
        ro = RobustRotationEstimatorOptions()
        ro.max_num_l1_iterations = 0
        ro.max_num_irls_iterations = io.max_num_irls_iterations
        ro.irls_step_convergence_threshold = io.irls_step_convergence_threshold
        ro.irls_loss_parameter_sigma = io.irls_loss_parameter_sigma
        # the views without a pair are outside the IRLS system: they are held as well
        live = np.zeros(len(ids), dtype=bool)
        live[np.unique(edges)] = True
        fixed = ~live
        fixed[ids.index(self._ld.gauge_view)] = True
        aa = np.array([result[v] for v in ids])
        rc, out, s = robust_rotation_averaging(aa, edges, rel, fixed, ro)
        if rc not in (0, capi.THEIA_HIP_ERR_INTERNAL):
            capi.check(rc)
        self.last_success = rc == 0
        self.last_irls_summary = s
        return {v: out[k].copy() for k, v in enumerate(ids)}


class NonlinearRotationEstimatorOptions:
    """ceres::Solver::Options as NonlinearRotationEstimator leaves them (nonlinear_rotation_estimator.cc:90-92), and the
    loss width of its constructor.  The reference's class exposes only the width; the rest is here so that every
    stopping rule can be reached."""

    def __init__(self):
        self.robust_loss_width = 0.1
        self.max_num_iterations = 200
        self.function_tolerance = 1e-6
        self.gradient_tolerance = 1e-10
        self.parameter_tolerance = 1e-8
        self.max_trust_region_radius = 1e16

    def to_c(self):
        o = capi.NonlinearRotationOptions()
        o.max_num_iterations = int(self.max_num_iterations)
        o.robust_loss_width = float(self.robust_loss_width)
        o.function_tolerance = float(self.function_tolerance)
        o.gradient_tolerance = float(self.gradient_tolerance)
        o.parameter_tolerance = float(self.parameter_tolerance)
        o.max_trust_region_radius = float(self.max_trust_region_radius)
        return o


def nonlinear_rotations(orientations, edges, relative_rotations, fixed=None, options=None, want_trace=False):
    """theia_hip_nonlinear_rotations on arrays: orientations [n][3] angle-axis (not modified), edges [E][2] view indices,
    relative_rotations [E][3] = TwoViewInfo::rotation_2, fixed: [n] booleans or None (no view held, the reference's
    problem).  Returns (return code, new orientations [n][3], NonlinearRotationSummary) and, with want_trace, the trace
    [rows][5] = (cost, gradient max norm, step norm, radius, accepted) as a fourth entry.  The orientations are the input
    on a refusal and after a FAILURE termination, the last accepted iterate otherwise."""
    o = (options or NonlinearRotationEstimatorOptions()).to_c()
    aa = np.array(orientations, dtype=np.float64).reshape(-1, 3)
    e, r = _pair_arrays(edges, relative_rotations, "relative rotation")
    f = None if fixed is None else np.ascontiguousarray(np.asarray(fixed, dtype=bool).astype(np.uint8))
    if f is not None and f.shape != (aa.shape[0],):
        raise ValueError("fixed must have one entry per view")
    rows = max(0, int(o.max_num_iterations)) + 1 if want_trace else 0
    trace = np.zeros((rows, 5)) if want_trace else None
    s = capi.NonlinearRotationSummary()
    rc = capi.lib().theia_hip_nonlinear_rotations(aa.shape[0], capi.ptr(aa, C.c_double), capi.ptr(f, C.c_uint8), e.shape[0],
                                                  capi.ptr(e, C.c_int32), capi.ptr(r, C.c_double), C.byref(o), C.byref(s),
                                                  capi.ptr(trace, C.c_double), rows)
    if want_trace:
        return rc, aa, s, trace[:s.trace_size].copy()
    return rc, aa, s


class NonlinearRotationEstimator:
    """NonlinearRotationEstimator(robust_loss_width=0.1) with EstimateRotations(view_pairs, orientations) -> dict
    (sfm.cc:1782-1787 -> nonlinear_rotation_estimator.{h,cc}), in RobustRotationEstimator's conventions: the input dict
    is not modified and the dict comes back whatever the outcome, the reference's bool is in last_success.

    Every pair whose two views both have an orientation adds one residual; a pair that lacks one is skipped silently
    (:76-80).  With no orientation, no pair, or no pair left (Ceres then has nothing to solve), last_success is False
    for the first two as in the reference (:53-62) and for the third as well, and the input comes back.  No view is held
    (DESIGN.md 3.6i on the gauge).  The constraints do not accumulate: the reference's class keeps no state."""

    def __init__(self, robust_loss_width=0.1):
        self.options = NonlinearRotationEstimatorOptions()
        self.options.robust_loss_width = float(robust_loss_width)
        self.last_summary = None
        self.last_success = None

    def EstimateRotations(self, view_pairs, orientations):
        result = {int(v): np.asarray(r, dtype=np.float64).reshape(3).copy() for v, r in orientations.items()}
        ids = list(result)
        pos = {v: k for k, v in enumerate(ids)}
        kept = [((int(a), int(b)), info) for (a, b), info in view_pairs.items() if int(a) in pos and int(b) in pos]
        self.last_summary = capi.NonlinearRotationSummary()
        if not ids or not kept:
            self.last_success = False
            return result
        edges = np.array([(pos[a], pos[b]) for (a, b), _ in kept], dtype=np.int32)
        rel = np.array([np.asarray(info.rotation_2, dtype=np.float64).reshape(3) for _, info in kept])
        aa = np.array([result[v] for v in ids])
        rc, out, s = nonlinear_rotations(aa, edges, rel, None, self.options)
        capi.check(rc)
        self.last_success = True
        self.last_summary = s
        return {v: out[k].copy() for k, v in enumerate(ids)}


def OrientationsFromMaximumSpanningTree(view_pairs):
    """OrientationsFromMaximumSpanningTree (view_graph/orientations_from_maximum_spanning_tree.cc:109-180) on the
    {(id1, id2): TwoViewInfo} dict that stands in for the ViewGraph: the largest connected component, its maximum
    spanning tree on num_verified_matches, the root at the zero vector, and every other view of the component chained
    along the tree: R_rel R_source when source id < neighbour id, R_rel' R_source otherwise (:74-77; a pair is stored
    under (smaller id, larger id) in the ViewGraph, and so it is read here whichever way the key names it -- a key
    (larger, smaller) is taken as that pair).  Host code, as in the reference.  Returns {view id: angle-axis}; a view
    outside the component gets no entry; an empty dict gives an empty dict.

    Where the reference follows hash order, two rules make the result a function of the graph alone:
      * the root is the smallest view id of the component (the reference: the first view of its unordered_set of tree
        edges); among components of equal size the one holding the smallest view id is taken;
      * the tree is Kruskal's over the pairs sorted by (-num_verified_matches, smaller id, larger id): among equal
        weights the pair with the smaller ids wins, whatever the order of the dict.
    Another root changes the result by a common rotation on the right, another tree among equal weights by the tree.
    The order in which the reference's heap visits the tree does not matter: a view's orientation is the product along
    its tree path."""
    pairs = {}
    for (a, b), info in view_pairs.items():
        a, b = int(a), int(b)
        if a != b:
            pairs[(min(a, b), max(a, b))] = info
    if not pairs:
        return {}
    parent = {}

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v

    for a, b in pairs:
        parent.setdefault(a, a)
        parent.setdefault(b, b)
    for a, b in pairs:
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)       # a component's representative is its smallest view id
    members = {}
    for v in parent:
        members.setdefault(find(v), []).append(v)
    root = min(members, key=lambda c: (-len(members[c]), c))
    component = set(members[root])
    # Kruskal, maximum weight first
    tree = {v: v for v in component}

    def find_t(v):
        while tree[v] != v:
            tree[v] = tree[tree[v]]
            v = tree[v]
        return v

    neighbours = {v: [] for v in component}
    for (a, b) in sorted((p for p in pairs if p[0] in component),
                         key=lambda p: (-int(pairs[p].num_verified_matches), p[0], p[1])):
        ra, rb = find_t(a), find_t(b)
        if ra != rb:
            tree[ra] = rb
            neighbours[a].append(b)
            neighbours[b].append(a)
    out = {root: np.zeros(3)}
    R = {root: np.eye(3)}
    stack = [root]
    while stack:
        src = stack.pop()
        for nb in neighbours[src]:
            if nb in R:
                continue
            Rrel = angle_axis_to_matrix(np.asarray(pairs[(min(src, nb), max(src, nb))].rotation_2, dtype=np.float64).reshape(3))
            R[nb] = (Rrel if src < nb else Rrel.T) @ R[src]
            out[nb] = _matrix_to_angle_axis(R[nb])
            stack.append(nb)
    return out


def _matrix_to_angle_axis(R):
    """ceres::RotationMatrixToAngleAxis (through the quaternion, as Ceres 2.2)."""
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    q = np.zeros(4)
    if tr >= 0.0:
        t = math.sqrt(tr + 1.0)
        q[0] = 0.5 * t
        t = 0.5 / t
        q[1], q[2], q[3] = (R[2, 1] - R[1, 2]) * t, (R[0, 2] - R[2, 0]) * t, (R[1, 0] - R[0, 1]) * t
    else:
        i = 0
        if R[1, 1] > R[0, 0]:
            i = 1
        if R[2, 2] > R[i, i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        t = math.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0)
        q[i + 1] = 0.5 * t
        t = 0.5 / t
        q[0] = (R[k, j] - R[j, k]) * t
        q[j + 1] = (R[j, i] + R[i, j]) * t
        q[k + 1] = (R[k, i] + R[i, k]) * t
    s2 = float(q[1:] @ q[1:])
    if s2 > 0.0:
        st = math.sqrt(s2)
        two_theta = 2.0 * (math.atan2(-st, -q[0]) if q[0] < 0.0 else math.atan2(st, q[0]))
        return q[1:] * (two_theta / st)
    return q[1:] * 2.0


class GlobalPositionEstimatorType(enum.IntEnum):  # reconstruction_estimator_options.h:80-85 (pybind sfm.cc:1196-1204)
    # all four on the device: NONLINEAR (NonlinearPositionEstimator, the reference's default), LINEAR_TRIPLET
    # (LinearPositionEstimator), LEAST_UNSQUARED_DEVIATION (LeastUnsquaredDeviationPositionEstimator), LIGT
    # (LiGTPositionEstimator)
    NONLINEAR = 0
    LINEAR_TRIPLET = 1
    LEAST_UNSQUARED_DEVIATION = 2
    LIGT = 3


class LeastUnsquaredDeviationPositionEstimatorOptions:  # least_unsquared_deviation_position_estimator.h:60-69
    def __init__(self):
        self.max_num_iterations = 400
        self.max_num_reweighted_iterations = 10
        self.convergence_criterion = 1e-4


class ConstrainedL1SolverOptions:  # math/constrained_l1_solver.h:64-74: what the estimator actually solves with
    def __init__(self):
        self.max_num_iterations = 1000
        self.rho = 10.0
        self.alpha = 1.2
        self.absolute_tolerance = 1e-4
        self.relative_tolerance = 1e-2

    def to_c(self):
        o = capi.LudOptions()
        o.max_num_iterations = int(self.max_num_iterations)
        o.rho = float(self.rho)
        o.alpha = float(self.alpha)
        o.absolute_tolerance = float(self.absolute_tolerance)
        o.relative_tolerance = float(self.relative_tolerance)
        return o


def lud_positions(orientations, edges, relative_translations, fixed=None, options=None, positions_out=None):
    """The C-ABI on arrays: orientations [n][3] angle-axis, edges [E][2] view indices, relative_translations [E][3]
    (TwoViewInfo::position_2), fixed: [n] booleans or None (view 0 held), options: ConstrainedL1SolverOptions.
    Returns (return code, positions [n][3], LudSummary); on a refusal the positions are positions_out (or zeros) as
    passed in, untouched."""
    o = (options or ConstrainedL1SolverOptions()).to_c()
    aa = np.ascontiguousarray(np.asarray(orientations, dtype=np.float64).reshape(-1, 3))
    e = np.ascontiguousarray(np.asarray(edges, dtype=np.int32).reshape(-1, 2))
    t = np.ascontiguousarray(np.asarray(relative_translations, dtype=np.float64).reshape(-1, 3))
    f = None if fixed is None else np.ascontiguousarray(np.asarray(fixed, dtype=bool).astype(np.uint8))
    if f is not None and f.shape != (aa.shape[0],):
        raise ValueError("fixed must have one entry per view")
    if t.shape[0] != e.shape[0]:
        raise ValueError("one relative translation per edge")
    out = np.zeros((aa.shape[0], 3)) if positions_out is None else positions_out
    if out.shape != (aa.shape[0], 3) or out.dtype != np.float64 or not out.flags["C_CONTIGUOUS"]:
        raise ValueError("positions_out must be a C-contiguous float64 [n][3] array")
    s = capi.LudSummary()
    rc = capi.lib().theia_hip_lud_positions(aa.shape[0], capi.ptr(aa, capi.C.c_double), capi.ptr(f, capi.C.c_uint8),
                                            e.shape[0], capi.ptr(e, capi.C.c_int32), capi.ptr(t, capi.C.c_double),
                                            capi.C.byref(o), capi.ptr(out, capi.C.c_double), capi.C.byref(s))
    return rc, out, s


class LeastUnsquaredDeviationPositionEstimator:
    """LeastUnsquaredDeviationPositionEstimator(options) with EstimatePositions(view_pairs, orientations) -> dict, as
    pyTheia binds it.  view_pairs: {(id1, id2): TwoViewInfo} (position_2 is read); orientations: {view_id: angle-axis}.

    The views are those of the pairs whose two views both have an orientation, in the order the pairs first name them;
    the first of them is held at the origin (the reference holds the first view of its unordered_set: the positions
    differ by a translation only).  A pair naming a view without an orientation is refused, as the
    reference's CHECK on the factorisation fails for it (its scale column stays empty)."""

    def __init__(self, options):
        # the constructor's CHECK_GTs are the only readers of these options: the reference solves with
        # ConstrainedL1Solver::Options at their defaults (:108-110) and so does this mirror
        if not options.max_num_iterations > 0:
            raise capi.TheiaHipError(capi.THEIA_HIP_ERR_INVALID_ARGUMENT, "max_num_iterations must be > 0")
        if not options.max_num_reweighted_iterations > 0:
            raise capi.TheiaHipError(capi.THEIA_HIP_ERR_INVALID_ARGUMENT, "max_num_reweighted_iterations must be > 0")
        self.options = options
        self.solver_options = ConstrainedL1SolverOptions()
        self.last_summary = None

    def EstimatePositions(self, view_pairs, orientations):
        if not view_pairs:
            raise capi.TheiaHipError(capi.THEIA_HIP_ERR_INVALID_ARGUMENT, "no view pairs")
        ids = {}
        for a, b in view_pairs:
            if int(a) in orientations and int(b) in orientations:
                ids.setdefault(int(a), len(ids))
                ids.setdefault(int(b), len(ids))
        for a, b in view_pairs:
            if int(a) not in ids or int(b) not in ids:
                raise capi.TheiaHipError(capi.THEIA_HIP_ERR_INVALID_ARGUMENT,
                                         f"view pair ({a}, {b}) names a view without an orientation")
        views = list(ids)
        edges = np.array([(ids[int(a)], ids[int(b)]) for a, b in view_pairs], dtype=np.int32)
        rel = np.array([np.asarray(info.position_2, dtype=np.float64).reshape(3) for info in view_pairs.values()])
        aa = np.array([np.asarray(orientations[v], dtype=np.float64).reshape(3) for v in views])
        fixed = np.arange(len(views)) == 0
        rc, pos, s = lud_positions(aa, edges, rel, fixed, self.solver_options)
        capi.check(rc)
        self.last_summary = s
        return {v: pos[k].copy() for k, v in enumerate(views)}


class LiGTPositionEstimatorOptions:  # LiGT_position_estimator.h:70-82
    def __init__(self):
        self.num_threads = 1              # held and ignored: the tracks are lanes and wavefronts of the launches
        self.max_power_iterations = 1000  # the reference declares these two and reads neither; here they stop the
        self.eigensolver_threshold = 1e-8  # inverse iteration
        self.max_num_views_svd = 500      # held and ignored: one dense Cholesky at every size

    def to_c(self):
        o = capi.LigtOptions()
        o.max_power_iterations = int(self.max_power_iterations)
        o.eigensolver_threshold = float(self.eigensolver_threshold)
        return o


def ligt_positions(orientations, track_offsets, obs_view, obs_feature, edges=None, relative_translations=None,
                   options=None, positions_out=None, want=()):
    """theia_hip_ligt_positions on arrays: orientations [n][3] angle-axis, track t = observations track_offsets[t] ..
    track_offsets[t + 1] - 1 of obs_view [N] / obs_feature [N][2] (normalised), edges [E][2] view indices with
    relative_translations [E][3] (TwoViewInfo::position_2) for the sign vote, or None.  want: names of the optional
    outputs to fetch, out of "base_pairs", "system", "system_index".  Returns (return code, positions [n][3], estimated
    [n] bool, LigtSummary, dict of the outputs asked for); a view outside the system keeps its positions_out row (zeros
    without positions_out); on a refusal nothing is written and the dict is empty."""
    o = (options or LiGTPositionEstimatorOptions()).to_c()
    aa = np.ascontiguousarray(np.asarray(orientations, dtype=np.float64).reshape(-1, 3))
    off = np.ascontiguousarray(np.asarray(track_offsets, dtype=np.int32).reshape(-1))
    ov = np.ascontiguousarray(np.asarray(obs_view, dtype=np.int32).reshape(-1))
    of = np.ascontiguousarray(np.asarray(obs_feature, dtype=np.float64).reshape(-1, 2))
    if off.shape[0] < 1:
        raise ValueError("track_offsets needs num_tracks + 1 entries")
    if ov.shape[0] != of.shape[0] or (off.shape[0] > 1 and int(off.max()) > ov.shape[0]):
        raise ValueError("one view and one feature per observation, and offsets within them")
    e = np.zeros((0, 2), dtype=np.int32) if edges is None else np.asarray(edges, dtype=np.int32).reshape(-1, 2)
    t = np.zeros((0, 3)) if relative_translations is None else np.asarray(relative_translations, dtype=np.float64).reshape(-1, 3)
    e, t = np.ascontiguousarray(e), np.ascontiguousarray(t)
    if t.shape[0] != e.shape[0]:
        raise ValueError("one relative translation per edge")
    unknown = set(want) - {"base_pairs", "system", "system_index"}
    if unknown:
        raise ValueError(f"unknown outputs {sorted(unknown)}")
    n, T = aa.shape[0], off.shape[0] - 1
    out = np.zeros((n, 3)) if positions_out is None else positions_out
    if out.shape != (n, 3) or out.dtype != np.float64 or not out.flags["C_CONTIGUOUS"]:
        raise ValueError("positions_out must be a C-contiguous float64 [n][3] array")
    est = np.zeros(n, dtype=np.uint8)
    bufs = {}
    if "base_pairs" in want:
        bufs["base_pairs"] = np.full((T, 2), -1, dtype=np.int32)
    if "system" in want:   # sized for every view in the system; cut to [3 (m - 1)]^2 below
        bufs["system"] = np.zeros(max(1, 3 * (n - 1)) ** 2)
    if "system_index" in want:
        bufs["system_index"] = np.full(n, -2, dtype=np.int32)
    s = capi.LigtSummary()
    rc = capi.lib().theia_hip_ligt_positions(
        n, capi.ptr(aa, C.c_double), T, capi.ptr(off, C.c_int32), capi.ptr(ov, C.c_int32), capi.ptr(of, C.c_double),
        e.shape[0], capi.ptr(e, C.c_int32), capi.ptr(t, C.c_double), C.byref(o), capi.ptr(out, C.c_double),
        capi.ptr(est, C.c_uint8), capi.ptr(bufs.get("base_pairs"), C.c_int32), capi.ptr(bufs.get("system"), C.c_double),
        capi.ptr(bufs.get("system_index"), C.c_int32), C.byref(s))
    if rc == 0 and "system" in bufs:
        k = 3 * (s.num_views_in_system - 1)
        bufs["system"] = bufs["system"][:k * k].reshape(k, k).copy()
    return rc, out, est.astype(bool), s, (bufs if rc == 0 else {})


def _pinhole_normalized(intrinsics, uv):
    """Camera::PixelToNormalizedCoordinates(pixel).hnormalized() of the pinhole model on arrays
    (ransac.Camera.pixel_to_normalized, observation by observation): intrinsics [N][>= 7], uv [N][2]."""
    f, a, sk, cx, cy, k1, k2 = (intrinsics[:, k] for k in range(7))
    y = (uv[:, 1] - cy) / (f * a)
    x = (uv[:, 0] - cx - y * sk) / f
    ux, uy = x.copy(), y.copy()
    active = np.ones(len(x), dtype=bool)
    for _ in range(100):
        if not active.any():
            break
        r2 = ux * ux + uy * uy
        d = 1.0 + r2 * (k1 + k2 * r2)
        nx, ny = x / d, y / d
        moved = (np.abs(nx - ux) >= 1e-10) | (np.abs(ny - uy) >= 1e-10)
        ux = np.where(active, nx, ux); uy = np.where(active, ny, uy)
        active &= moved
    return np.column_stack([ux, uy])


class _TrackPositionEstimator:
    """What the position estimators that read the tracks share (LiGTPositionEstimator, LinearPositionEstimator): the
    reconstruction's observations as the array calls take them.  The tracks are taken in increasing id and a track's
    observations in the order the reconstruction lists them (the reference walks hash containers).
    normalized_features [N][2]: the observations' hnormalized(PixelToNormalizedCoordinates(pixel)); without it the pixels
    of pinhole groups are un-projected here and any other model raises, as ransac.Camera.pixel_to_normalized does.  An
    observation of a view without an orientation raises (the reference's lookups throw or die)."""

    def __init__(self, options, reconstruction, normalized_features=None):
        if not options.num_threads > 0:   # CHECK_GT(options.num_threads, 0)
            raise capi.TheiaHipError(capi.THEIA_HIP_ERR_INVALID_ARGUMENT, "num_threads must be > 0")
        self.options = options
        self.reconstruction = reconstruction
        self.normalized_features = normalized_features
        self.last_summary = None

    def _features(self):
        r = self.reconstruction
        if self.normalized_features is not None:
            f = np.asarray(self.normalized_features, dtype=np.float64).reshape(-1, 2)
            if f.shape[0] != len(r.obs_view):
                raise ValueError("one normalized feature per observation")
            return f
        groups = np.asarray(r.view_group)[r.obs_view]
        if np.any(np.asarray(r.group_model)[groups] != 0):
            raise capi.TheiaHipError(capi.THEIA_HIP_ERR_UNSUPPORTED,
                                     "pixel_to_normalized mirrors the pinhole model only; pass normalized_features for the others")
        return _pinhole_normalized(np.asarray(r.group_intrinsics, dtype=np.float64)[groups],
                                   np.asarray(r.obs_uv, dtype=np.float64).reshape(-1, 2))

    def _track_arrays(self, orientations):
        """(views: the ids with an orientation, sorted; pos: id -> index; orientations [n][3]; track_offsets; obs_view as
        indices; obs_feature), the last three in track order."""
        r = self.reconstruction
        ov = np.asarray(r.obs_view, dtype=np.int64)
        ot = np.asarray(r.obs_track, dtype=np.int64)
        feats = self._features()
        missing = sorted({int(v) for v in np.unique(ov)} - {int(v) for v in orientations})
        if missing:
            raise capi.TheiaHipError(capi.THEIA_HIP_ERR_INVALID_ARGUMENT, f"view {missing[0]} has no orientation")
        views = sorted(int(v) for v in orientations)
        pos = {v: k for k, v in enumerate(views)}
        lut = np.full(max(views) + 1 if views else 1, -1, dtype=np.int64)
        lut[views] = np.arange(len(views))
        order = np.argsort(ot, kind="stable")   # tracks in increasing id, observations in the reconstruction's order
        ntracks = r.NumTracks()
        offsets = np.concatenate([[0], np.cumsum(np.bincount(ot, minlength=ntracks))]).astype(np.int32)
        aa = np.array([np.asarray(orientations[v], dtype=np.float64).reshape(3) for v in views]).reshape(-1, 3)
        return views, pos, aa, offsets, lut[ov[order]], feats[order]


class LiGTPositionEstimator(_TrackPositionEstimator):
    """LiGTPositionEstimator(options, reconstruction) with EstimatePositions(view_pairs, orientations) -> dict, as
    pyTheia binds it.  reconstruction: the array-backed sfm.Reconstruction (obs_view, obs_track and obs_uv are read; ids
    are dense indices); view_pairs: {(id1, id2): TwoViewInfo}, whose position_2 only votes on the sign; orientations:
    {view_id: angle-axis}.

    The tracks are taken in increasing id and a track's observations in the order the reconstruction lists them
    (the reference walks hash containers).  normalized_features [N][2]: the observations'
    hnormalized(PixelToNormalizedCoordinates(pixel)); without it the pixels of pinhole groups are un-projected here and any
    other model raises, as ransac.Camera.pixel_to_normalized does.  An observation of a view without an orientation
    raises (the reference's orientations_.at() throws).  The dict holds the views of the system: those of the tracks
    that were used."""

    def EstimatePositions(self, view_pairs, orientations):
        views, pos, aa, offsets, ov, feats = self._track_arrays(orientations)
        keys = [k for k in view_pairs if int(k[0]) in pos and int(k[1]) in pos]
        edges = np.array([(pos[int(a)], pos[int(b)]) for a, b in keys], dtype=np.int32).reshape(-1, 2)
        rel = np.array([np.asarray(view_pairs[k].position_2, dtype=np.float64).reshape(3) for k in keys]).reshape(-1, 3)
        rc, p, est, s, _ = ligt_positions(aa, offsets, ov, feats, edges, rel, self.options)
        capi.check(rc)
        self.last_summary = s
        return {v: p[k].copy() for k, v in enumerate(views) if est[k]}


class LinearPositionEstimatorOptions:  # linear_position_estimator.h
    def __init__(self):
        self.num_threads = 1              # held and ignored (checked > 0): the triangles are wavefronts of the launches
        self.max_power_iterations = 1000  # the reference declares these two and reads neither; here they stop the
        self.eigensolver_threshold = 1e-8  # inverse iteration

    def to_c(self):
        o = capi.LinearTripletOptions()
        o.max_power_iterations = int(self.max_power_iterations)
        o.eigensolver_threshold = float(self.eigensolver_threshold)
        return o


LINEAR_TRIPLET_OUTPUTS = ("triplets", "triplet_state", "baselines", "system", "system_index")


def linear_triplet_positions(orientations, edges, relative_rotations, relative_translations, track_offsets, obs_view,
                             obs_feature, options=None, positions_out=None, want=(), triplet_capacity=None):
    """theia_hip_linear_triplet_positions on arrays: orientations [n][3] angle-axis, edges [E][2] view indices with first <
    second, relative_rotations / relative_translations [E][3] (TwoViewInfo::rotation_2 / position_2), track t =
    observations track_offsets[t] .. track_offsets[t + 1] - 1 of obs_view [N] / obs_feature [N][2] (normalised).  want:
    names of the optional outputs to fetch, out of LINEAR_TRIPLET_OUTPUTS; the three per-triangle ones hold the first
    triplet_capacity triangles (default: room for every triangle the view pairs could form, E (n - 2) / 3 at most, capped
    at 2^20).  Returns (return code, positions [n][3], estimated [n] bool, LinearTripletSummary, dict of the outputs asked
    for); a view outside the system keeps its positions_out row (zeros without positions_out); on a refusal nothing is
    written and the dict is empty."""
    o = (options or LinearPositionEstimatorOptions()).to_c()
    aa = np.ascontiguousarray(np.asarray(orientations, dtype=np.float64).reshape(-1, 3))
    e, rr = _pair_arrays(edges, relative_rotations, "relative rotation")
    _, rt = _pair_arrays(edges, relative_translations, "relative translation")
    off = np.ascontiguousarray(np.asarray(track_offsets, dtype=np.int32).reshape(-1))
    ov = np.ascontiguousarray(np.asarray(obs_view, dtype=np.int32).reshape(-1))
    of = np.ascontiguousarray(np.asarray(obs_feature, dtype=np.float64).reshape(-1, 2))
    if off.shape[0] < 1:
        raise ValueError("track_offsets needs num_tracks + 1 entries")
    if ov.shape[0] != of.shape[0] or (off.shape[0] > 1 and int(off.max()) > ov.shape[0]):
        raise ValueError("one view and one feature per observation, and offsets within them")
    unknown = set(want) - set(LINEAR_TRIPLET_OUTPUTS)
    if unknown:
        raise ValueError(f"unknown outputs {sorted(unknown)}")
    n, E, T = aa.shape[0], e.shape[0], off.shape[0] - 1
    out = np.zeros((n, 3)) if positions_out is None else positions_out
    if out.shape != (n, 3) or out.dtype != np.float64 or not out.flags["C_CONTIGUOUS"]:
        raise ValueError("positions_out must be a C-contiguous float64 [n][3] array")
    est = np.zeros(n, dtype=np.uint8)
    per_triangle = {"triplets", "triplet_state", "baselines"} & set(want)
    cap = 0
    if per_triangle:
        cap = min(E * max(0, n - 2) // 3, 1 << 20) if triplet_capacity is None else int(triplet_capacity)
    bufs = {}
    if "triplets" in want:
        bufs["triplets"] = np.full((cap, 3), -1, dtype=np.int32)
    if "triplet_state" in want:
        bufs["triplet_state"] = np.full(cap, 255, dtype=np.uint8)
    if "baselines" in want:
        bufs["baselines"] = np.zeros((cap, 3))
    if "system" in want:   # sized for every view in the system; cut to [3 (m - 1)]^2 below
        bufs["system"] = np.zeros(max(1, 3 * (n - 1)) ** 2)
    if "system_index" in want:
        bufs["system_index"] = np.full(n, -2, dtype=np.int32)
    s = capi.LinearTripletSummary()
    rc = capi.lib().theia_hip_linear_triplet_positions(
        n, capi.ptr(aa, C.c_double), E, capi.ptr(e, C.c_int32), capi.ptr(rr, C.c_double), capi.ptr(rt, C.c_double),
        T, capi.ptr(off, C.c_int32), capi.ptr(ov, C.c_int32), capi.ptr(of, C.c_double), C.byref(o),
        capi.ptr(out, C.c_double), capi.ptr(est, C.c_uint8), cap, capi.ptr(bufs.get("triplets"), C.c_int32),
        capi.ptr(bufs.get("triplet_state"), C.c_uint8), capi.ptr(bufs.get("baselines"), C.c_double),
        capi.ptr(bufs.get("system"), C.c_double), capi.ptr(bufs.get("system_index"), C.c_int32), C.byref(s))
    if rc == 0:
        if "system" in bufs:
            k = 3 * (s.num_views_in_system - 1)
            bufs["system"] = bufs["system"][:k * k].reshape(k, k).copy()
        head = min(cap, s.num_triplets)
        for name in per_triangle:
            bufs[name] = bufs[name][:head].copy()
    return rc, out, est.astype(bool), s, (bufs if rc == 0 else {})


class LinearPositionEstimator(_TrackPositionEstimator):
    """LinearPositionEstimator(options, reconstruction) with EstimatePositions(view_pairs, orientations) -> dict, as
    pyTheia binds it.  reconstruction: the array-backed sfm.Reconstruction (obs_view, obs_track and obs_uv are read; ids
    are dense indices); view_pairs: {(id1, id2): TwoViewInfo} keyed id1 < id2, whose rotation_2 and position_2 are read;
    orientations: {view_id: angle-axis}.  Tracks, ids and un-projection as LiGTPositionEstimator takes them.  A pair or
    an observation naming a view without an orientation raises (the reference's FindOrDie).  The dict holds the views of
    the system: those of the largest component of triangles."""

    def EstimatePositions(self, view_pairs, orientations):
        views, pos, aa, offsets, ov, feats = self._track_arrays(orientations)
        for a, b in view_pairs:
            for v in (a, b):
                if int(v) not in pos:
                    raise capi.TheiaHipError(capi.THEIA_HIP_ERR_INVALID_ARGUMENT,
                                             f"view pair ({a}, {b}) names view {v}, which has no orientation")
            if not int(a) < int(b):
                raise capi.TheiaHipError(capi.THEIA_HIP_ERR_INVALID_ARGUMENT, f"view pair ({a}, {b}) is not keyed id1 < id2")
        keys = list(view_pairs)
        edges = np.array([(pos[int(a)], pos[int(b)]) for a, b in keys], dtype=np.int32).reshape(-1, 2)
        rot = np.array([np.asarray(view_pairs[k].rotation_2, dtype=np.float64).reshape(3) for k in keys]).reshape(-1, 3)
        rel = np.array([np.asarray(view_pairs[k].position_2, dtype=np.float64).reshape(3) for k in keys]).reshape(-1, 3)
        rc, p, est, s, _ = linear_triplet_positions(aa, edges, rot, rel, offsets, ov, feats, self.options)
        capi.check(rc)
        self.last_summary = s
        return {v: p[k].copy() for k, v in enumerate(views) if est[k]}


class NonlinearPositionEstimatorOptions:  # nonlinear_position_estimator.h:63-82
    def __init__(self):
        self.rng = None                   # a ransac.RandomNumberGenerator; None: one seeded from the clock at construction
        self.num_threads = 1              # held and ignored (checked > 0): the edges are lanes of the launches
        self.max_num_iterations = 400
        self.robust_loss_width = 0.1
        self.min_num_points_per_view = 0
        self.point_to_camera_weight = 0.5
        # ceres::Solver::Options as the reference leaves them; here so that every stopping rule can be reached
        self.function_tolerance = 1e-6
        self.gradient_tolerance = 1e-10
        self.parameter_tolerance = 1e-8
        self.max_trust_region_radius = 1e16

    def to_c(self):
        o = capi.NonlinearPositionOptions()
        o.max_num_iterations = int(self.max_num_iterations)
        o.robust_loss_width = float(self.robust_loss_width)
        o.function_tolerance = float(self.function_tolerance)
        o.gradient_tolerance = float(self.gradient_tolerance)
        o.parameter_tolerance = float(self.parameter_tolerance)
        o.max_trust_region_radius = float(self.max_trust_region_radius)
        return o


def nonlinear_positions(orientations, positions, edges, relative_translations, scale_estimates=None, fixed=None,
                        points=None, track_offsets=None, obs_view=None, obs_feature=None, ray_orientations=None,
                        point_to_camera_weight=0.5, options=None, want_trace=False):
    """theia_hip_nonlinear_positions on arrays: orientations [n][3] angle-axis, positions [n][3] the start (not
    modified), edges [E][2] view indices with relative_translations [E][3] = TwoViewInfo::position_2 and scale_estimates
    [E] or None (all -1), fixed: [n] booleans or None (no view held).  points [T][3] the start of the track points (not
    modified) with track t = observations track_offsets[t] .. track_offsets[t + 1] - 1 of obs_view [N] / obs_feature
    [N][2] (normalised), or None: no point part; ray_orientations [n][3] or None (= orientations).
    point_to_camera_weight is the weight of every point-to-camera edge as the call takes it (the estimator class scales
    the option by the edge counts first).  Returns (return code, new positions [n][3], new points [T][3],
    NonlinearPositionSummary) and, with want_trace, the trace [rows][5] = (cost, gradient max norm, step norm, radius,
    accepted) as a fifth entry.  Positions and points are the input on a refusal and after a FAILURE termination, the
    last accepted iterate otherwise."""
    o = (options or NonlinearPositionEstimatorOptions()).to_c()
    aa = np.ascontiguousarray(np.asarray(orientations, dtype=np.float64).reshape(-1, 3))
    x = np.array(positions, dtype=np.float64).reshape(-1, 3)
    n = aa.shape[0]
    if x.shape[0] != n:
        raise ValueError("one position per view")
    e, r = _pair_arrays(np.zeros((0, 2), dtype=np.int32) if edges is None else edges,
                        np.zeros((0, 3)) if relative_translations is None else relative_translations, "relative translation")
    se = None if scale_estimates is None else np.ascontiguousarray(np.asarray(scale_estimates, dtype=np.float64).reshape(-1))
    if se is not None and se.shape[0] != e.shape[0]:
        raise ValueError("one scale estimate per edge")
    f = None if fixed is None else np.ascontiguousarray(np.asarray(fixed, dtype=bool).astype(np.uint8))
    if f is not None and f.shape != (n,):
        raise ValueError("fixed must have one entry per view")
    ray = None if ray_orientations is None else np.ascontiguousarray(np.asarray(ray_orientations, dtype=np.float64).reshape(-1, 3))
    if ray is not None and ray.shape[0] != n:
        raise ValueError("one ray orientation per view")
    pts = off = ov = of = None
    T = 0
    if points is not None:
        pts = np.array(points, dtype=np.float64).reshape(-1, 3)
        T = pts.shape[0]
        off = np.ascontiguousarray(np.asarray(track_offsets, dtype=np.int32).reshape(-1))
        ov = np.ascontiguousarray(np.asarray(obs_view, dtype=np.int32).reshape(-1))
        of = np.ascontiguousarray(np.asarray(obs_feature, dtype=np.float64).reshape(-1, 2))
        if off.shape[0] != T + 1:
            raise ValueError("track_offsets needs num_points + 1 entries")
        if ov.shape[0] != of.shape[0] or int(off.max()) > ov.shape[0]:
            raise ValueError("one view and one feature per observation, and offsets within them")
    rows = max(0, int(o.max_num_iterations)) + 1 if want_trace else 0
    trace = np.zeros((rows, 5)) if want_trace else None
    s = capi.NonlinearPositionSummary()
    rc = capi.lib().theia_hip_nonlinear_positions(
        n, capi.ptr(aa, C.c_double), capi.ptr(x, C.c_double), capi.ptr(f, C.c_uint8), e.shape[0], capi.ptr(e, C.c_int32),
        capi.ptr(r, C.c_double), capi.ptr(se, C.c_double), T, capi.ptr(pts if T else None, C.c_double),
        capi.ptr(off, C.c_int32), capi.ptr(ov, C.c_int32), capi.ptr(of, C.c_double), capi.ptr(ray, C.c_double),
        float(point_to_camera_weight), C.byref(o), C.byref(s), capi.ptr(trace, C.c_double), rows)
    if pts is None:
        pts = np.zeros((0, 3))
    if want_trace:
        return rc, x, pts, s, trace[:s.trace_size].copy()
    return rc, x, pts, s


class NonlinearPositionEstimator(_TrackPositionEstimator):
    """NonlinearPositionEstimator(options, reconstruction) with EstimatePositions(view_pairs, orientations) -> dict,
    SetViewsFixed(view_ids) and EstimateRemainingPositionsInRecon(fixed_views, views_in_subrecon, view_pairs) ->
    (bool, dict) (global_pose_estimation/nonlinear_position_estimator.{h,cc}).  reconstruction: the array-backed
    sfm.Reconstruction (ids are dense indices); view_pairs: {(id1, id2): TwoViewInfo}, whose position_2 and scale_estimate
    are read; orientations: {view_id: angle-axis}.  The reference's bool is in last_success (the solution is usable:
    any termination but FAILURE), the summary in last_summary, the points of the selected tracks in
    triangulated_points.

    Host logic as the reference's; where it walks a hash container a stated rule stands in:
      * empty pairs or orientations: last_success = False and {} (:141-145);
      * random start (:208-224), when no view is fixed: every view with an orientation that a pair names gets
        100 * RandVector3d(), three RandDouble(-1, 1) draws taken as x, y, z, from options.rng (or the generator seeded
        from the clock at construction); the views are taken in increasing id; the stream is left where the draws end;
      * a pair lacking a position on either side is skipped (:235-238); the pairs are taken in the dict's order;
      * track selection (:297-380) with min_num_points_per_view > 0: the positioned views in increasing id, a view with
        fewer features than the minimum skipped, its tracks not yet selected ordered by (-number of views, track id),
        and taken from the front until the view has its minimum; each taken track counts toward every positioned view
        that sees it.  The weight of a point-to-camera edge is point_to_camera_weight * (camera edges) / (sum of the
        per-view counts); with a zero sum there is no point part;
      * an estimated selected track starts at points[t][:3] / points[t][3] and adds one edge per observation of a
        positioned view, its ray turned by the view's own stored orientation, reconstruction.cam_ext[:, 3:6] (the
        reference's GetRotatedFeatureRay, :68-75, sets the solve's orientation on a temporary and then asks the
        original camera); an un-estimated one draws its three random numbers and adds no edge (:279-287); the tracks
        are taken in increasing id;
      * gauge (:168-176): with no fixed view the smallest positioned view id is set to zero and recorded as fixed, not
        held, so the first solve holds nothing; a later call on the same object holds that view and skips the random
        start, and needs the view's position: through EstimatePositions there is none, the reference's FindOrDie, and
        INVALID_ARGUMENT is raised."""

    def __init__(self, options, reconstruction, normalized_features=None):
        super().__init__(options, reconstruction, normalized_features)   # CHECK_GT(options.num_threads, 0)
        if not options.min_num_points_per_view >= 0:
            raise capi.TheiaHipError(capi.THEIA_HIP_ERR_INVALID_ARGUMENT, "min_num_points_per_view must be >= 0")
        if not options.point_to_camera_weight > 0:
            raise capi.TheiaHipError(capi.THEIA_HIP_ERR_INVALID_ARGUMENT, "point_to_camera_weight must be > 0")
        if not options.robust_loss_width > 0:
            raise capi.TheiaHipError(capi.THEIA_HIP_ERR_INVALID_ARGUMENT, "robust_loss_width must be > 0")
        from . import ransac
        self._rng = options.rng if options.rng is not None else ransac.RandomNumberGenerator()
        self._fixed = set()
        self.triangulated_points = {}
        self.last_success = None

    def SetViewsFixed(self, fixed_views):
        self._fixed = {int(v) for v in fixed_views}

    def EstimatePositions(self, view_pairs, orientations):
        return self._estimate(view_pairs, orientations, {})

    def EstimateRemainingPositionsInRecon(self, fixed_views, views_in_subrecon, view_pairs):
        r = self.reconstruction
        ids = sorted(int(v) for v in views_in_subrecon if 0 <= int(v) < r.NumViews())
        orientations = {v: np.array(r.cam_ext[v, 3:6], dtype=np.float64) for v in ids}
        positions = {v: np.array(r.cam_ext[v, :3], dtype=np.float64) for v in ids}
        self._fixed = {int(v) for v in fixed_views}
        out = self._estimate(view_pairs, orientations, positions)
        return self.last_success, out

    def _random_vector(self):
        return 100.0 * np.array([self._rng.RandDouble(-1.0, 1.0) for _ in range(3)])

    def _find_tracks(self, positions):
        """FindTracksForProblem: ({track: estimated} in selection order, the sum of the per-view counts)."""
        r, k = self.reconstruction, int(self.options.min_num_points_per_view)
        ov = np.asarray(r.obs_view, dtype=np.int64)
        ot = np.asarray(r.obs_track, dtype=np.int64)
        nv, nt = r.NumViews(), r.NumTracks()
        views_of = np.bincount(ot, minlength=nt)
        by_view, by_track = np.argsort(ov, kind="stable"), np.argsort(ot, kind="stable")
        view_off = np.concatenate([[0], np.cumsum(np.bincount(ov, minlength=nv))])
        track_off = np.concatenate([[0], np.cumsum(views_of)])
        per_view = {v: 0 for v in positions}
        chosen = {}
        for v in sorted(positions):
            if not 0 <= v < nv:
                continue
            mine = ot[by_view[view_off[v]:view_off[v + 1]]]
            if len(mine) < k:
                continue
            cand = sorted((int(t) for t in mine if int(t) not in chosen), key=lambda t: (-int(views_of[t]), t))[:k]
            for t in cand:
                if per_view[v] >= k:
                    break
                chosen[t] = bool(r.track_estimated[t])
                for w in ov[by_track[track_off[t]:track_off[t + 1]]]:
                    if int(w) in per_view:
                        per_view[int(w)] += 1
        return chosen, sum(per_view.values())

    def _estimate(self, view_pairs, orientations, positions):
        self.last_summary = capi.NonlinearPositionSummary()
        self.triangulated_points = {}
        if not view_pairs or not orientations:
            self.last_success = False
            return {}
        orientations = {int(v): np.asarray(w, dtype=np.float64).reshape(3) for v, w in orientations.items()}
        positions = {int(v): np.asarray(p, dtype=np.float64).reshape(3).copy() for v, p in positions.items()}
        if not self._fixed:
            named = {int(v) for pair in view_pairs for v in pair}
            for v in sorted(orientations):
                if v in named:
                    positions[v] = self._random_vector()
        views = sorted(positions)
        index = {v: k for k, v in enumerate(views)}
        kept = [(int(a), int(b), info) for (a, b), info in view_pairs.items() if int(a) in index and int(b) in index]
        missing = sorted(v for v in views if v not in orientations)
        if missing:                     # FindOrDie(orientations, view_id)
            raise capi.TheiaHipError(capi.THEIA_HIP_ERR_INVALID_ARGUMENT, f"view {missing[0]} has no orientation")
        edges = np.array([(index[a], index[b]) for a, b, _ in kept], dtype=np.int32).reshape(-1, 2)
        rel = np.array([np.asarray(info.position_2, dtype=np.float64).reshape(3) for _, _, info in kept]).reshape(-1, 3)
        scales = np.array([float(info.scale_estimate) for _, _, info in kept])
        point_args, tracks, weight = {}, [], float(self.options.point_to_camera_weight)
        if self.options.min_num_points_per_view > 0:
            chosen, count = self._find_tracks(positions)
            if count > 0:
                weight = weight * float(len(kept)) / float(count)
                r = self.reconstruction
                feats = self._features()
                ov = np.asarray(r.obs_view, dtype=np.int64)
                ot = np.asarray(r.obs_track, dtype=np.int64)
                start, offsets, obs_v, obs_f = [], [0], [], []
                by_track = np.argsort(ot, kind="stable")
                track_off = np.concatenate([[0], np.cumsum(np.bincount(ot, minlength=r.NumTracks()))])
                for t in sorted(chosen):
                    if not chosen[t]:
                        self.triangulated_points[t] = self._random_vector()
                        continue
                    self.triangulated_points[t] = np.array(r.points[t][:3] / r.points[t][3], dtype=np.float64)
                    rows = [k for k in by_track[track_off[t]:track_off[t + 1]] if int(ov[k]) in index]
                    if not rows:
                        continue
                    tracks.append(t)
                    start.append(self.triangulated_points[t])
                    obs_v += [index[int(ov[k])] for k in rows]
                    obs_f += [feats[k] for k in rows]
                    offsets.append(len(obs_v))
                if tracks:
                    ray = np.array([np.asarray(r.cam_ext[v, 3:6], dtype=np.float64) if 0 <= v < r.NumViews()
                                    else orientations[v] for v in views])
                    point_args = dict(points=np.array(start), track_offsets=offsets, obs_view=obs_v,
                                      obs_feature=np.array(obs_f).reshape(-1, 2), ray_orientations=ray)
        fixed = None
        if not self._fixed:
            if views:
                positions[views[0]] = np.zeros(3)
                self._fixed.add(views[0])
        else:
            missing = sorted(v for v in self._fixed if v not in index)
            if missing:                 # FindOrDie(*positions, v_id)
                raise capi.TheiaHipError(capi.THEIA_HIP_ERR_INVALID_ARGUMENT, f"fixed view {missing[0]} has no position")
            fixed = np.array([v in self._fixed for v in views])
        if not kept and not tracks:     # Ceres has nothing to solve
            self.last_success = False
            return positions
        aa = np.array([orientations[v] for v in views])
        x0 = np.array([positions[v] for v in views])
        rc, x, pts, s = nonlinear_positions(aa, x0, edges, rel, scales, fixed, point_to_camera_weight=weight,
                                            options=self.options, **point_args)
        capi.check(rc)
        self.last_summary = s
        self.last_success = s.termination != capi.ROTATION_TERM_FAILURE
        for k, t in enumerate(tracks):
            self.triangulated_points[t] = pts[k].copy()
        return {v: x[k].copy() for k, v in enumerate(views)}


class FilterViewPairsFromRelativeTranslationOptions:  # filter_view_pairs_from_relative_translation.h:48-66
    def __init__(self):
        self.rng = None           # a ransac.RandomNumberGenerator; None: a generator seeded from the clock per call
        self.num_threads = 1      # held and ignored: the iterations are workgroups of one launch
        self.num_iterations = 48
        self.translation_projection_tolerance = 0.08

    def to_c(self):
        o = capi.TranslationFilterOptions()
        o.num_iterations = int(self.num_iterations)
        o.translation_projection_tolerance = float(self.translation_projection_tolerance)
        return o


def _pair_arrays(pairs, per_pair, what):
    e = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
    t = np.ascontiguousarray(np.asarray(per_pair, dtype=np.float64).reshape(-1, 3))
    if t.shape[0] != e.shape[0]:
        raise ValueError(f"one {what} per pair")
    return e, t


def filter_translations_1dsfm(orientations, pairs, position_2, options=None, rng_state=None, axes=None, want=()):
    """theia_hip_filter_view_pairs_from_relative_translation on arrays: orientations [n][3] angle-axis, pairs [E][2] view
    indices (every unordered pair at most once), position_2 [E][3].  rng_state: the capi.RngState the axes are drawn
    from and that the call advances; axes: [num_iterations][3] unit vectors used instead.  want: names of the optional
    outputs to fetch, out of "bad_weight", "order", "axes", "rotated".  Returns (return code, removed [E] bool, dict of
    the outputs asked for); on a refusal removed is all False and the dict is empty."""
    o = (options or FilterViewPairsFromRelativeTranslationOptions()).to_c()
    aa = np.ascontiguousarray(np.asarray(orientations, dtype=np.float64).reshape(-1, 3))
    e, t = _pair_arrays(pairs, position_2, "position_2")
    n, E, iters = aa.shape[0], e.shape[0], max(0, o.num_iterations)
    ax = None
    if axes is not None:
        ax = np.ascontiguousarray(np.asarray(axes, dtype=np.float64).reshape(-1, 3))
        if ax.shape[0] != iters:
            raise ValueError("one axis per iteration")
    unknown = set(want) - {"bad_weight", "order", "axes", "rotated"}
    if unknown:
        raise ValueError(f"unknown outputs {sorted(unknown)}")
    removed = np.zeros(E, dtype=np.uint8)
    bufs = dict(bad_weight=np.zeros(E), order=np.full((iters, n), -1, dtype=np.int32), axes=np.full((iters, 3), np.nan),
                rotated=np.zeros((E, 3)))
    arg = lambda k, ct: capi.ptr(bufs[k] if k in want else None, ct)
    rc = capi.lib().theia_hip_filter_view_pairs_from_relative_translation(
        n, E, capi.ptr(e, C.c_int32), capi.ptr(aa, C.c_double), capi.ptr(t, C.c_double), C.byref(o),
        None if rng_state is None else C.byref(rng_state), capi.ptr(ax, C.c_double), capi.ptr(removed, C.c_uint8),
        arg("bad_weight", C.c_double), arg("order", C.c_int32), arg("axes", C.c_double), arg("rotated", C.c_double))
    return rc, removed.astype(bool), ({k: bufs[k] for k in want} if rc == 0 else {})


def translation_filter_last_stats():
    """theia_hip_translation_filter_last_stats of the calling thread, as a dict."""
    s = capi.TranslationFilterStats()
    capi.check(capi.lib().theia_hip_translation_filter_last_stats(C.byref(s)))
    return {name: getattr(s, name) for name, _ in s._fields_}


def filter_pairs_from_orientation(orientations, pairs, rotation_2, max_relative_rotation_difference_degrees,
                                  has_orientation=None):
    """theia_hip_filter_view_pairs_from_orientation on arrays: rotation_2 [E][3] = TwoViewInfo::rotation_2,
    has_orientation: [n] booleans or None.  Returns (return code, removed [E] bool)."""
    aa = np.ascontiguousarray(np.asarray(orientations, dtype=np.float64).reshape(-1, 3))
    e, r = _pair_arrays(pairs, rotation_2, "rotation_2")
    h = None if has_orientation is None else np.ascontiguousarray(np.asarray(has_orientation, dtype=bool).astype(np.uint8))
    if h is not None and h.shape != (aa.shape[0],):
        raise ValueError("has_orientation must have one entry per view")
    removed = np.zeros(e.shape[0], dtype=np.uint8)
    rc = capi.lib().theia_hip_filter_view_pairs_from_orientation(
        aa.shape[0], e.shape[0], capi.ptr(e, C.c_int32), capi.ptr(aa, C.c_double), capi.ptr(h, C.c_uint8),
        capi.ptr(r, C.c_double), float(max_relative_rotation_difference_degrees), capi.ptr(removed, C.c_uint8))
    return rc, removed.astype(bool)


def _graph_views(view_pairs):
    """The views the pairs name, in increasing id: the filters' "lowest view index" is the lowest view id."""
    views = sorted({int(v) for pair in view_pairs for v in pair})
    return views, {v: k for k, v in enumerate(views)}


def FilterViewPairsFromRelativeTranslation(options, orientations, view_pairs):
    """FilterViewPairsFromRelativeTranslation(options, orientations, view_graph) with the {(id1, id2): TwoViewInfo} dict
    in the ViewGraph's place: the removed pairs are deleted from it and their number is returned.  The axes come from
    options.rng, i.e. the calling thread's generator, which is left where the draws end; options.rng = None seeds that
    generator from the clock first, as the reference's per-thread RandomNumberGenerator() does."""
    from . import ransac
    views, pos = _graph_views(view_pairs)
    keys = list(view_pairs)
    aa = np.zeros((len(views), 3))
    for a, _ in keys:   # FindOrDie(orientations, view_pair.first.first): only a pair's first view is looked up
        if int(a) not in orientations:
            raise capi.TheiaHipError(capi.THEIA_HIP_ERR_INVALID_ARGUMENT, f"view {a} has no orientation")
    for v in views:
        if v in orientations:
            aa[pos[v]] = np.asarray(orientations[v], dtype=np.float64).reshape(3)
    pairs = np.array([(pos[int(a)], pos[int(b)]) for a, b in keys], dtype=np.int32).reshape(-1, 2)
    rel = np.array([np.asarray(view_pairs[k].position_2, dtype=np.float64).reshape(3) for k in keys]).reshape(-1, 3)
    rng = options.rng if options.rng is not None else ransac.RandomNumberGenerator()
    rc, removed, _ = filter_translations_1dsfm(aa, pairs, rel, options, rng_state=rng.thread_state())
    capi.check(rc)
    for k, gone in zip(keys, removed):
        if gone:
            del view_pairs[k]
    return int(removed.sum())


def FilterViewPairsFromOrientation(orientations, max_relative_rotation_difference_degrees, view_pairs):
    """FilterViewPairsFromOrientation(orientations, max degrees, view_graph) on the dict: a pair whose rotation_2
    disagrees with the two orientations by more than the angle, or that names a view without an orientation, is deleted;
    returns how many were."""
    views, pos = _graph_views(view_pairs)
    keys = list(view_pairs)
    aa = np.zeros((len(views), 3))
    has = np.zeros(len(views), dtype=bool)
    for v in views:
        if v in orientations:
            aa[pos[v]] = np.asarray(orientations[v], dtype=np.float64).reshape(3)
            has[pos[v]] = True
    pairs = np.array([(pos[int(a)], pos[int(b)]) for a, b in keys], dtype=np.int32).reshape(-1, 2)
    rel = np.array([np.asarray(view_pairs[k].rotation_2, dtype=np.float64).reshape(3) for k in keys]).reshape(-1, 3)
    rc, removed = filter_pairs_from_orientation(aa, pairs, rel, max_relative_rotation_difference_degrees, has)
    capi.check(rc)
    for k, gone in zip(keys, removed):
        if gone:
            del view_pairs[k]
    return int(removed.sum())


def filter_cycles_by_rotation(num_views, pairs, rotation_2, max_loop_error_degrees, want=()):
    """theia_hip_filter_view_graph_cycles_by_rotation on arrays: pairs [E][2] view indices (every unordered pair at most
    once, in either order), rotation_2 [E][3] of the pair as listed.  want: names of the optional outputs to fetch, out of
    "min_loop_error_degrees" [E], "triangles_per_pair" [E] and "num_triangles" (an int).  Returns (return code, removed
    [E] bool, dict of the outputs asked for); on a refusal removed is all False and the dict is empty."""
    e, r = _pair_arrays(pairs, rotation_2, "rotation_2")
    unknown = set(want) - {"min_loop_error_degrees", "triangles_per_pair", "num_triangles"}
    if unknown:
        raise ValueError(f"unknown outputs {sorted(unknown)}")
    E = e.shape[0]
    removed = np.zeros(E, dtype=np.uint8)
    bufs = dict(min_loop_error_degrees=np.full(E, np.inf), triangles_per_pair=np.zeros(E, dtype=np.int32),
                num_triangles=np.zeros(1, dtype=np.int64))
    arg = lambda k, ct: capi.ptr(bufs[k] if k in want else None, ct)
    rc = capi.lib().theia_hip_filter_view_graph_cycles_by_rotation(
        int(num_views), E, capi.ptr(e, C.c_int32), capi.ptr(r, C.c_double), float(max_loop_error_degrees),
        capi.ptr(removed, C.c_uint8), arg("min_loop_error_degrees", C.c_double), arg("triangles_per_pair", C.c_int32),
        arg("num_triangles", C.c_int64))
    bufs["num_triangles"] = int(bufs["num_triangles"][0])
    return rc, removed.astype(bool), ({k: bufs[k] for k in want} if rc == 0 else {})


def remove_disconnected_pairs(num_views, pairs):
    """theia_hip_remove_disconnected_view_pairs on arrays (host code: no device is touched).  Returns (return code,
    removed_pairs [E] bool, removed_views [num_views] bool, component [num_views] int32: the smallest view index of the
    view's component, -1 for a view no pair names); on a refusal nothing is marked and component is all -1."""
    e = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
    n = int(num_views)
    removed_pairs = np.zeros(e.shape[0], dtype=np.uint8)
    removed_views = np.zeros(max(n, 0), dtype=np.uint8)
    component = np.full(max(n, 0), -1, dtype=np.int32)
    rc = capi.lib().theia_hip_remove_disconnected_view_pairs(
        n, e.shape[0], capi.ptr(e, C.c_int32), capi.ptr(removed_pairs, C.c_uint8), capi.ptr(removed_views, C.c_uint8),
        capi.ptr(component, C.c_int32))
    return rc, removed_pairs.astype(bool), removed_views.astype(bool), component


def FilterViewGraphCyclesByRotation(max_loop_error_degrees, view_pairs):
    """FilterViewGraphCyclesByRotation(max_loop_error_degrees, view_graph) on the dict: a pair that lies in no triangle
    whose chained rotations close to within the angle is deleted; returns how many were.  A key (id2, id1) with
    id2 > id1 is taken as listed: its rotation_2 belongs to that orientation."""
    views, pos = _graph_views(view_pairs)
    keys = list(view_pairs)
    pairs = np.array([(pos[int(a)], pos[int(b)]) for a, b in keys], dtype=np.int32).reshape(-1, 2)
    rel = np.array([np.asarray(view_pairs[k].rotation_2, dtype=np.float64).reshape(3) for k in keys]).reshape(-1, 3)
    rc, removed, _ = filter_cycles_by_rotation(len(views), pairs, rel, max_loop_error_degrees)
    capi.check(rc)
    for k, gone in zip(keys, removed):
        if gone:
            del view_pairs[k]
    return int(removed.sum())


def RemoveDisconnectedViewPairs(view_pairs):
    """RemoveDisconnectedViewPairs(view_graph) on the dict: the pairs outside the largest connected component (among
    equally large ones, the one with the smallest view id stays) are deleted; returns the set of the removed view ids,
    as the binding does."""
    views, pos = _graph_views(view_pairs)
    keys = list(view_pairs)
    pairs = np.array([(pos[int(a)], pos[int(b)]) for a, b in keys], dtype=np.int32).reshape(-1, 2)
    rc, removed_pairs, removed_views, _ = remove_disconnected_pairs(len(views), pairs)
    capi.check(rc)
    for k, gone in zip(keys, removed_pairs):
        if gone:
            del view_pairs[k]
    return {v for v, gone in zip(views, removed_views) if gone}
