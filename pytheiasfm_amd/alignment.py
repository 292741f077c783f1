"""Host-side mirror of pyTheia's reconstruction alignment (src/theia/sfm/transformation/, exported in
src/pytheia/sfm/sfm.cc:620-628,938) over theia_hip_align_point_clouds, theia_hip_transform_reconstruction and the RANSAC
estimator THEIA_EST_CAMERA_ALIGNMENT (include/theia_hip.h), and of the Sim(3) optimisation (sfm.cc:631-670) over
theia_hip_optimize_alignment_sim3 and theia_hip_sim3_maps, and the Sim(3) pose graph of camera poses
(pose_graph_sim3_error.h, Sim3Manifold of align_reconstructions_pose_graph_optim.{h,cc}) over theia_hip_pose_graph_sim3
(the reference has no driver for it, so the names from OptimizePoseGraphSim3 on are this library's).

Same names as the pybind wrappers; the Align* functions return (rotation [3][3], translation [3], scale).  Reconstructions are
the array-backed pytheiasfm_amd.sfm.Reconstruction; the functions that match views by name need its `view_names`."""
import ctypes as C
import enum

import numpy as np

from . import _capi as capi
from . import ransac as _ransac


def _invalid(message):
    return capi.TheiaHipError(capi.THEIA_HIP_ERR_INVALID_ARGUMENT, message)


def _cloud(a, name):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.ndim != 2 or a.shape[1] != 3:
        raise _invalid(f"{name}: an [n][3] array of points is needed")
    return a


def align_point_clouds_batch(lefts, rights, weights=None, timings=None):
    """theia_hip_align_point_clouds on lists of clouds.  Returns (rotation [P][3][3], translation [P][3], scale [P], status
    [P]); status is capi.THEIA_ALIGN_OK or capi.THEIA_ALIGN_DEGENERATE (identity returned, as the reference does with a
    warning).  timings: an optional list that receives [kernel ms, call ms]."""
    lefts = [_cloud(a, "left") for a in lefts]
    rights = [_cloud(a, "right") for a in rights]
    P = len(lefts)
    if len(rights) != P or (weights is not None and len(weights) != P):
        raise _invalid("left, right and weights must hold one entry per problem")
    ws = None
    if weights is not None:
        ws = [np.ascontiguousarray(w, dtype=np.float64).reshape(-1) for w in weights]
    for p in range(P):   # CHECK_EQ(left.size(), right.size()), CHECK_EQ(left.size(), weights.size())
        if lefts[p].shape[0] != rights[p].shape[0] or (ws is not None and ws[p].shape[0] != lefts[p].shape[0]):
            raise _invalid(f"problem {p}: left, right and weights differ in length")
    R = np.zeros((max(P, 1), 3, 3)); t = np.zeros((max(P, 1), 3)); s = np.zeros(max(P, 1)); st = np.zeros(max(P, 1), dtype=np.int32)
    if P == 0:
        return R[:0], t[:0], s[:0], st[:0]
    offsets = np.concatenate([[0], np.cumsum([a.shape[0] for a in lefts])]).astype(np.int64)
    left = np.ascontiguousarray(np.concatenate(lefts)); right = np.ascontiguousarray(np.concatenate(rights))
    w = None if ws is None else np.ascontiguousarray(np.concatenate(ws))
    tm = None if timings is None else np.zeros(2)
    capi.check(capi.lib().theia_hip_align_point_clouds(
        P, capi.ptr(offsets, C.c_int64), capi.ptr(left, C.c_double), capi.ptr(right, C.c_double), capi.ptr(w, C.c_double),
        capi.ptr(R, C.c_double), capi.ptr(t, C.c_double), capi.ptr(s, C.c_double), capi.ptr(st, C.c_int32),
        capi.ptr(tm, C.c_double)))
    if timings is not None:
        timings[:] = tm.tolist()
    return R, t, s, st


def AlignPointCloudsUmeyamaBatch(lefts, rights):
    """AlignPointCloudsUmeyama for a list of pairs in one call: a list of (rotation, translation, scale)."""
    R, t, s, _ = align_point_clouds_batch(lefts, rights)
    return [(R[p].copy(), t[p].copy(), float(s[p])) for p in range(len(s))]


def AlignPointCloudsUmeyamaWithWeightsBatch(lefts, rights, weights):
    """AlignPointCloudsUmeyamaWithWeights for a list of pairs in one call: a list of (rotation, translation, scale)."""
    R, t, s, _ = align_point_clouds_batch(lefts, rights, weights)
    return [(R[p].copy(), t[p].copy(), float(s[p])) for p in range(len(s))]


def AlignPointCloudsUmeyama(left, right):
    """align_point_clouds.cc:45-54 -> (rotation, translation, scale) with right ~ scale * rotation * left + translation."""
    return AlignPointCloudsUmeyamaBatch([left], [right])[0]


def AlignPointCloudsUmeyamaWithWeights(left, right, weights):
    """align_point_clouds.cc:56-150 -> (rotation, translation, scale)."""
    return AlignPointCloudsUmeyamaWithWeightsBatch([left], [right], [weights])[0]


def _transform(R, t, s):
    R = np.ascontiguousarray(R, dtype=np.float64); t = np.ascontiguousarray(t, dtype=np.float64).reshape(-1)
    if R.shape != (3, 3) or t.shape != (3,):
        raise _invalid("a 3 x 3 rotation and a translation of 3 are needed")
    return R, t, float(s)


def TransformReconstruction(reconstruction, rotation, translation, scale, timings=None):
    """transform_reconstruction.cc:73-94, in place: estimated views' cameras (position s R c + t, orientation R_cam R^T) and
    estimated tracks' points (hnormalized, s R p + t, w = 1).  As in the reference, tracks' inverse depths and reference bearing
    vectors are not touched."""
    R, t, s = _transform(rotation, translation, scale)
    r = reconstruction
    cams = np.ascontiguousarray(r.cam_ext, dtype=np.float64).reshape(-1, 6)
    pts = np.ascontiguousarray(r.points, dtype=np.float64).reshape(-1, 4)
    cm = np.ascontiguousarray(r.view_estimated, dtype=np.uint8).reshape(-1)
    pm = np.ascontiguousarray(r.track_estimated, dtype=np.uint8).reshape(-1)
    if cm.shape[0] != cams.shape[0] or pm.shape[0] != pts.shape[0]:
        raise _invalid("view_estimated / track_estimated do not match the cameras / points")
    tm = None if timings is None else np.zeros(2)
    capi.check(capi.lib().theia_hip_transform_reconstruction(
        cams.shape[0], capi.ptr(cams, C.c_double), capi.ptr(cm, C.c_uint8), pts.shape[0], capi.ptr(pts, C.c_double),
        capi.ptr(pm, C.c_uint8), capi.ptr(R, C.c_double), capi.ptr(t, C.c_double), s, capi.ptr(tm, C.c_double)))
    if timings is not None:
        timings[:] = tm.tolist()
    if cams is not r.cam_ext:
        r.cam_ext = cams
    if pts is not r.points:
        r.points = pts


def TransformReconstruction4(reconstruction, T):
    """transform_reconstruction.cc:96-102: rotation = T[:3, :3], translation = T[:3, 3], scale = T[3, 3]."""
    T = np.asarray(T, dtype=np.float64)
    if T.shape != (4, 4):
        raise _invalid("a 4 x 4 transformation is needed")
    TransformReconstruction(reconstruction, T[:3, :3], T[:3, 3], T[3, 3])


def _names(reconstruction):
    names = getattr(reconstruction, "view_names", None)
    if names is None:
        raise _invalid("the reconstruction has no view_names")
    if len(names) != reconstruction.NumViews():
        raise _invalid("view_names must hold one name per view")
    return list(names)


def FindCommonViewsByName(reconstruction1, reconstruction2):
    """find_common_views_by_name.cc: the names of the views both reconstructions hold.  STATED ORDER: reconstruction1's view
    order (the reference walks an unordered_map: hash order)."""
    n2 = set(_names(reconstruction2))
    return [n for n in _names(reconstruction1) if n in n2]


def _common_positions(rec1, rec2):
    common = FindCommonViewsByName(rec1, rec2)
    id1 = {n: i for i, n in enumerate(_names(rec1))}
    id2 = {n: i for i, n in enumerate(_names(rec2))}
    i1 = np.array([id1[n] for n in common], dtype=np.int64); i2 = np.array([id2[n] for n in common], dtype=np.int64)
    return np.asarray(rec1.cam_ext)[i1, :3].reshape(-1, 3), np.asarray(rec2.cam_ext)[i2, :3].reshape(-1, 3)


def AlignReconstructions(reconstruction1, reconstruction2):
    """align_reconstructions.cc:97-131: Umeyama of the common views' positions, reconstruction2 -> reconstruction1, applied to
    reconstruction2 in place.  Returns (rotation, translation, scale)."""
    p1, p2 = _common_positions(reconstruction1, reconstruction2)
    if p1.shape[0] == 0:
        raise _invalid("the reconstructions have no view in common")   # the reference reads left[0]
    R, t, s = AlignPointCloudsUmeyama(p2, p1)
    TransformReconstruction(reconstruction2, R, t, s)
    return R, t, s


def AlignReconstructionsRobust(robust_error_threshold, reconstruction1, reconstruction2, seed=0, rng=None):
    """align_reconstructions.cc:133-197: RANSAC over the common views' positions with CameraAlignmentEstimator
    (max_iterations 1000, use_mle, error_thresh = threshold^2, failure_probability 1e-4, the rest at RansacParameters'
    defaults), Umeyama on its inliers, reconstruction2 transformed in place.  `seed` / `rng` reach the sampler as
    RansacParameters.seed / .rng do in the Estimate* mirrors.  Raises where the reference CHECKs: fewer common views than the
    sample, a failed estimate, no inliers.  Returns (rotation, translation, scale)."""
    p1, p2 = _common_positions(reconstruction1, reconstruction2)
    params = _ransac.RansacParameters()
    params.max_iterations = 1000
    params.use_mle = True
    params.error_thresh = float(robust_error_threshold) * float(robust_error_threshold)
    params.failure_probability = 1e-4
    params.seed = seed
    params.rng = rng
    data = np.ascontiguousarray(np.hstack([p1, p2]))
    ok, _, summary = _ransac._single(_ransac.EST_CAMERA_ALIGNMENT, params, _ransac.RansacType.RANSAC, data)
    if not ok:
        raise _invalid("Could not align models with RANSAC")
    if len(summary.inliers) == 0:
        raise _invalid("No inliers could be found for estimating the similarity transformation. Try using a higher error threshold.")
    inl = np.asarray(summary.inliers, dtype=np.int64)
    R, t, s = AlignPointCloudsUmeyama(p2[inl], p1[inl])
    TransformReconstruction(reconstruction2, R, t, s)
    return R, t, s


def align_rotations(gt_rotation, rotation, want_trace=False):
    """theia_hip_align_rotations -> (aligned rotations [n][3], alignment w [3], capi.AlignRotationsSummary, trace [rows][5] or
    None).  The inputs are not changed."""
    gt = np.ascontiguousarray(gt_rotation, dtype=np.float64).reshape(-1, 3)
    rot = np.array(rotation, dtype=np.float64).reshape(-1, 3)
    if gt.shape[0] != rot.shape[0]:
        raise _invalid("gt_rotation and rotation differ in length")   # CHECK_EQ(gt_rotation.size(), rotation->size())
    w = np.zeros(3)
    summ = capi.AlignRotationsSummary()
    rows = 64   # the start and at most 50 iterations
    trace = np.zeros((rows, 5)) if want_trace else None
    capi.check(capi.lib().theia_hip_align_rotations(rot.shape[0], capi.ptr(gt, C.c_double), capi.ptr(rot, C.c_double),
                                                    capi.ptr(w, C.c_double), C.byref(summ), capi.ptr(trace, C.c_double),
                                                    rows if want_trace else 0))
    return rot, w, summ, (trace[:summ.trace_size] if want_trace else None)


def AlignRotations(gt_rotation, rotation):
    """align_rotations.cc:127-156: the rotations (angle-axis, [n][3]) aligned to gt_rotation by one rotation on the right,
    rotation_i R ~ gt_rotation_i.  pyTheia returns the aligned vector; so does this."""
    return align_rotations(gt_rotation, rotation)[0]


def AlignOrientations(gt_orientations, orientations):
    """AlignOrientations as pyTheia binds it (math/rotation.cc:82-103 through math_wrapper.cc:5-12): AlignRotations over the
    view ids of gt_orientations, every one of which `orientations` must hold (the reference's FindOrDie); returns a copy of
    `orientations` with those entries aligned.  STATED ORDER: gt_orientations' own order (the reference walks an
    unordered_map); it only decides which residual block is which."""
    ids = list(gt_orientations)
    missing = [k for k in ids if k not in orientations]
    if missing or not ids:
        raise _invalid("orientations must hold every view of gt_orientations, and there must be one")
    aligned = AlignRotations([gt_orientations[k] for k in ids], [orientations[k] for k in ids])
    out = dict(orientations)
    for k, a in zip(ids, aligned):
        out[k] = a.copy()
    return out


# ---- Sim(3) point-cloud alignment (align_point_clouds.h:60-160, align_point_clouds.cc:161-317; sfm.cc:631-670)
class Sim3AlignmentType(enum.IntEnum):
    POINT_TO_POINT = capi.THEIA_SIM3_POINT_TO_POINT
    ROBUST_POINT_TO_POINT = capi.THEIA_SIM3_ROBUST_POINT_TO_POINT
    POINT_TO_PLANE = capi.THEIA_SIM3_POINT_TO_PLANE


POINT_TO_POINT = Sim3AlignmentType.POINT_TO_POINT                  # export_values()
ROBUST_POINT_TO_POINT = Sim3AlignmentType.ROBUST_POINT_TO_POINT
POINT_TO_PLANE = Sim3AlignmentType.POINT_TO_PLANE


class Sim3AlignmentOptions:
    """align_point_clouds.h:76-140 with its defaults.  outlier_threshold, linear_solver_type and verbose are kept and not read
    (the reference reads outlier_threshold nowhere; a single 7-block leaves the linear solver no choice); minimizer_type
    "LINE_SEARCH" is refused.  start_from_initial_alignment is not in the reference: see OptimizeAlignmentSim3."""

    def __init__(self):
        self.alignment_type = Sim3AlignmentType.POINT_TO_POINT
        self.point_weight = 1.0
        self.huber_threshold = 0.1
        self.outlier_threshold = 1.0
        self.linear_solver_type = "SPARSE_SCHUR"
        self.minimizer_type = "TRUST_REGION"
        self.max_iterations = 100
        self.verbose = False
        self.perform_optimization = True
        self.start_from_initial_alignment = False
        self.initial_sim3_params = None
        self.target_normals = None
        self.point_weights = None

    def set_initial_sim3_params(self, params):
        self.initial_sim3_params = np.array(params, dtype=np.float64).reshape(7)

    def set_target_normals(self, normals):
        self.target_normals = np.array(normals, dtype=np.float64).reshape(-1, 3)

    def set_point_weights(self, weights):
        self.point_weights = np.array(weights, dtype=np.float64).reshape(-1)

    def clear_initial_sim3_params(self):
        self.initial_sim3_params = None

    def clear_target_normals(self):
        self.target_normals = None

    def clear_point_weights(self):
        self.point_weights = None


class Sim3AlignmentSummary:
    """align_point_clouds.h:143-160, and what the device loop adds: termination (capi.THEIA_SIM3_TERM_*), initial_cost, the
    step counts and the trace rows (cost, gradient max norm, step norm, radius, accepted)."""

    def __init__(self):
        self.success = False
        self.final_cost = 0.0
        self.num_iterations = 0
        self.alignment_error = 0.0
        self.sim3_params = np.zeros(7)
        self.termination = capi.THEIA_SIM3_TERM_NO_POINTS
        self.initial_cost = 0.0
        self.num_successful_steps = self.num_unsuccessful_steps = self.num_invalid_steps = 0
        self.route = 0
        self.trace = None


def sim3_maps(op, values):
    """theia_hip_sim3_maps on an [n][in width] array -> [n][out width]."""
    wi, wo = capi.THEIA_SIM3_MAP_WIDTHS[op]
    v = np.ascontiguousarray(values, dtype=np.float64).reshape(-1, wi)
    out = np.zeros((v.shape[0], wo))
    capi.check(capi.lib().theia_hip_sim3_maps(op, v.shape[0], capi.ptr(v, C.c_double), capi.ptr(out, C.c_double)))
    return out


def Sim3FromRotationTranslationScale(rotation, translation, scale):
    """align_point_clouds.cc:288-298 -> the 7 parameters [upsilon, omega, sigma] of Sim3d(RxSO3d(scale, R), t).log()."""
    R, t, s = _transform(rotation, translation, scale)
    if not (1e-10 <= s < 1e10):
        raise _invalid("Scale factor must be greater-equal epsilon.")     # Sophus' SOPHUS_ENSURE
    return sim3_maps(capi.THEIA_SIM3_MAP_FROM_RTS, np.concatenate([R.reshape(-1), t, [s]]))[0]


def Sim3ToRotationTranslationScale(sim3_params):
    """align_point_clouds.cc:300-317 -> (rotation [3][3], translation [3], scale)."""
    o = sim3_maps(capi.THEIA_SIM3_MAP_TO_RTS, np.asarray(sim3_params, dtype=np.float64).reshape(1, 7))[0]
    return o[:9].reshape(3, 3).copy(), o[9:12].copy(), float(o[12])


def Sim3ToHomogeneousMatrix(sim3_params):
    """transformation_wrapper.cc:125-132 -> Sim3d::exp(params).matrix() [4][4]."""
    return sim3_maps(capi.THEIA_SIM3_MAP_TO_MATRIX4, np.asarray(sim3_params, dtype=np.float64).reshape(1, 7))[0].reshape(4, 4)


def optimize_alignment_sim3(sources, targets, starts, options, weights=None, normals=None, want_trace=False, timings=None):
    """theia_hip_optimize_alignment_sim3 on lists of clouds: problem p is sources[p] -> targets[p] from starts[p] under
    options[p] (Sim3AlignmentOptions: alignment_type, point_weight, huber_threshold, max_iterations are read).  weights /
    normals: None, or one array per problem (all problems or none: the C entry takes one array for the batch).
    Returns (params [P][7], [capi.Sim3AlignmentSummaryC], [trace [rows][5]] or None)."""
    P = len(sources)
    src = [_cloud(a, "source") for a in sources]
    tgt = [_cloud(a, "target") for a in targets]
    if len(tgt) != P or len(options) != P or len(starts) != P:
        raise _invalid("sources, targets, starts and options must hold one entry per problem")
    for p in range(P):
        if src[p].shape[0] != tgt[p].shape[0]:
            raise _invalid(f"problem {p}: source and target differ in length")
    offsets = np.concatenate([[0], np.cumsum([a.shape[0] for a in src])]).astype(np.int64)
    cat = lambda arrs, w: np.ascontiguousarray(np.concatenate([np.asarray(a, dtype=np.float64).reshape(-1, w) for a in arrs]) if arrs
                                               else np.zeros((0, w)))
    S, T = cat(src, 3), cat(tgt, 3)
    W = N = None
    if weights is not None:
        W = cat(weights, 1).reshape(-1)
        if W.shape[0] != S.shape[0]:
            raise _invalid("weights must hold one entry per point")
    if normals is not None:
        N = cat(normals, 3)
        if N.shape[0] != S.shape[0]:
            raise _invalid("normals must hold one entry per point")
    st = np.ascontiguousarray(np.asarray(starts, dtype=np.float64).reshape(P, 7))
    opts = (capi.Sim3AlignmentOptionsC * max(P, 1))()
    for p, o in enumerate(options):
        opts[p].alignment_type = int(o.alignment_type)
        opts[p].max_iterations = int(o.max_iterations)
        opts[p].point_weight = float(o.point_weight)
        opts[p].huber_threshold = float(o.huber_threshold)
    summ = (capi.Sim3AlignmentSummaryC * max(P, 1))()
    params = np.zeros((max(P, 1), 7))
    rows = (max((int(o.max_iterations) for o in options), default=0) + 2) if want_trace else 0
    trace = np.zeros((max(P, 1), rows, 5)) if want_trace else None
    tm = None if timings is None else np.zeros(2)
    capi.check(capi.lib().theia_hip_optimize_alignment_sim3(
        P, capi.ptr(offsets, C.c_int64), capi.ptr(S, C.c_double), capi.ptr(T, C.c_double), capi.ptr(W, C.c_double),
        capi.ptr(N, C.c_double), capi.ptr(st, C.c_double), opts, capi.ptr(params, C.c_double), summ,
        capi.ptr(trace, C.c_double), rows, capi.ptr(tm, C.c_double)))
    if timings is not None:
        timings[:] = tm.tolist()
    traces = [trace[p, :summ[p].trace_size].copy() for p in range(P)] if want_trace else None
    return params[:P], [summ[p] for p in range(P)], traces


_SIM3_AS_WRITTEN_START = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0])   # align_point_clouds.cc:178-179


def OptimizeAlignmentSim3Batch(sources, targets, options=None, want_trace=False):
    """OptimizeAlignmentSim3 for a list of cloud pairs: one launch for the problems that are optimised, one Umeyama call
    for those that need an initial alignment.  options: None, one Sim3AlignmentOptions for all, or one per pair.  A list of
    Sim3AlignmentSummary."""
    P = len(sources)
    if len(targets) != P:
        raise _invalid("sources and targets must hold one entry per problem")
    if options is None:
        options = Sim3AlignmentOptions()
    opts = list(options) if isinstance(options, (list, tuple)) else [options] * P
    if len(opts) != P:
        raise _invalid("one Sim3AlignmentOptions per problem is needed")
    out = [Sim3AlignmentSummary() for _ in range(P)]
    src = [np.asarray(a, dtype=np.float64).reshape(-1, 3) for a in sources]
    tgt = [np.asarray(a, dtype=np.float64).reshape(-1, 3) for a in targets]
    live = []
    for p, o in enumerate(opts):
        if str(getattr(o.minimizer_type, "name", o.minimizer_type)).upper() == "LINE_SEARCH":
            raise _invalid("minimizer_type LINE_SEARCH is not built")
        if src[p].shape[0] != tgt[p].shape[0] or src[p].shape[0] == 0:
            continue   # "must have the same size" / "cannot be empty" (:168-175): the summary as constructed
        live.append(p)
    # the initial alignment (:181-198): the guess, or weighted Umeyama (all ones) -> Sim3FromRotationTranslationScale
    need = [p for p in live if opts[p].initial_sim3_params is None]
    if need:
        R, t, s, _ = align_point_clouds_batch([src[p] for p in need], [tgt[p] for p in need],
                                              [np.ones(src[p].shape[0]) for p in need])
        rts = np.concatenate([R.reshape(len(need), 9), t, s[:, None]], axis=1)
        inside = (rts[:, 12] >= 1e-10) & (rts[:, 12] < 1e10)
        if not inside.all():
            raise _invalid("Scale factor must be greater-equal epsilon.")
        init = sim3_maps(capi.THEIA_SIM3_MAP_FROM_RTS, rts)
        for k, p in enumerate(need):
            out[p].sim3_params = init[k].copy()
    for p in live:
        if opts[p].initial_sim3_params is not None:
            out[p].sim3_params = np.array(opts[p].initial_sim3_params, dtype=np.float64).reshape(7)
        out[p].success = True
    run = [p for p in live if opts[p].perform_optimization]
    if not run:
        return out
    starts, W, N = [], [], []
    any_w = any(opts[p].point_weights is not None for p in run)
    any_n = any(opts[p].alignment_type == Sim3AlignmentType.POINT_TO_PLANE and opts[p].target_normals is not None for p in run)
    run_opts = []
    for p in run:
        o = opts[p]
        n = src[p].shape[0]
        starts.append(out[p].sim3_params if o.start_from_initial_alignment else _SIM3_AS_WRITTEN_START)
        w = np.full(n, float(o.point_weight))
        if o.point_weights is not None:   # `i < point_weights->size()` (:210-215): the points past its end take point_weight
            pw = np.asarray(o.point_weights, dtype=np.float64).reshape(-1)[:n]
            w[:pw.shape[0]] = pw
        W.append(w)
        ro = Sim3AlignmentOptions()
        ro.alignment_type, ro.point_weight = o.alignment_type, o.point_weight
        ro.huber_threshold, ro.max_iterations = o.huber_threshold, o.max_iterations
        nn = np.tile([0.0, 0.0, 1.0], (n, 1))
        if o.alignment_type == Sim3AlignmentType.POINT_TO_PLANE:
            tn = None if o.target_normals is None else np.asarray(o.target_normals, dtype=np.float64).reshape(-1, 3)
            if tn is None or tn.shape[0] < n:
                # no normals: point-to-point (:228-238).  (Normals for only some of the points -- the reference then mixes
                # both residual kinds in one problem -- are not built.)
                if tn is not None:
                    raise _invalid(f"problem {p}: target_normals must hold one normal per point")
                ro.alignment_type = Sim3AlignmentType.POINT_TO_POINT
            else:
                nn = tn[:n]
        N.append(nn)
        run_opts.append(ro)
    params, summ, traces = optimize_alignment_sim3([src[p] for p in run], [tgt[p] for p in run], starts, run_opts,
                                                   weights=W if any_w else None, normals=N if any_n else None,
                                                   want_trace=want_trace)
    for k, p in enumerate(run):
        c = summ[k]
        r = out[p]
        r.success = bool(c.success)                       # :269
        r.final_cost, r.initial_cost = c.final_cost, c.initial_cost
        r.num_iterations = c.num_iterations               # :271
        r.sim3_params = params[k].copy()                  # :272
        r.alignment_error = c.alignment_error             # :275-281
        r.termination, r.route = c.termination, c.route
        r.num_successful_steps, r.num_unsuccessful_steps = c.num_successful_steps, c.num_unsuccessful_steps
        r.num_invalid_steps = c.num_invalid_steps
        r.trace = traces[k] if want_trace else None
    return out


def OptimizeAlignmentSim3(source_points, target_points, options=None):
    """align_point_clouds.cc:161-284.  AS WRITTEN, the reference stores the initial alignment (the guess, or Umeyama) in the
    summary, then optimises a separate block that starts at (0,0,0,0,0,0,1) -- identity rotation, scale e -- and overwrites
    the summary with it (:178-198, :253, :272); so does this by default.  options.start_from_initial_alignment = True (a
    field the reference does not have) starts the solve at the initial alignment, as the reference's comments intend.
    A size mismatch or an empty cloud returns the summary as constructed (success False)."""
    return OptimizeAlignmentSim3Batch([source_points], [target_points], options)[0]


# ---- Sim(3) pose-graph optimisation of camera poses (theia_hip_pose_graph_sim3)
class Sim3PoseGraphOptions:
    """ceres::Solver::Options' defaults, the six numbers theia_pose_graph_sim3_options carries."""

    def __init__(self):
        self.max_num_iterations = 50
        self.function_tolerance = 1e-6
        self.gradient_tolerance = 1e-10
        self.parameter_tolerance = 1e-8
        self.initial_trust_region_radius = 1e4
        self.max_trust_region_radius = 1e16

    def to_c(self):
        o = capi.PoseGraphSim3OptionsC()
        o.max_num_iterations = int(self.max_num_iterations)
        o.function_tolerance, o.gradient_tolerance = float(self.function_tolerance), float(self.gradient_tolerance)
        o.parameter_tolerance = float(self.parameter_tolerance)
        o.initial_trust_region_radius = float(self.initial_trust_region_radius)
        o.max_trust_region_radius = float(self.max_trust_region_radius)
        return o


class Sim3PoseGraphSummary:
    """theia_pose_graph_sim3_summary; success as ceres::Solver::Summary::IsSolutionUsable (CONVERGENCE or NO_CONVERGENCE);
    trace [rows][5] = (cost, gradient max norm, step norm, radius, accepted) when asked for."""

    def __init__(self, c=None, trace=None):
        c = capi.PoseGraphSim3SummaryC() if c is None else c
        for name, _ in c._fields_:
            if name != "reserved":
                setattr(self, name, getattr(c, name))
        self.success = self.termination not in (capi.THEIA_SIM3_TERM_NO_POINTS, capi.THEIA_SIM3_TERM_FAILURE)
        self.trace = trace


def OptimizePoseGraphSim3(nodes, edges, measurements, sqrt_information=None, fixed=None, options=None, want_trace=False):
    """theia_hip_pose_graph_sim3: Levenberg-Marquardt over one Sim3ReconAlignErrorTerm (pose_graph_sim3_error.h:46-103) per
    edge (i, j), residual sqrt_information log(Sji exp(x_i) exp(x_j)^-1) with measurements = log(Sji), every node on
    Sim3Manifold, the nodes flagged in `fixed` held constant.  nodes [n][7] in Sophus' order upsilon | omega | sigma; edges
    [E][2]; measurements [E][7]; sqrt_information [E][7][7] or None (identity).  Returns (nodes [n][7], Sim3PoseGraphSummary);
    the input is not changed.  Not in the reference's scope here: SelfEdgesErrorTerm / CrossEdgesErrorTerm (a cross edge is
    an edge to a held node with an identity measurement), a robust loss."""
    x = np.array(nodes, dtype=np.float64, order="C")
    if x.ndim != 2 or x.shape[1] != 7:
        raise _invalid("nodes: an [n][7] array is needed")
    n = x.shape[0]
    e = np.ascontiguousarray(edges, dtype=np.int32).reshape(-1, 2)
    E = e.shape[0]
    z = np.ascontiguousarray(measurements, dtype=np.float64)
    if z.size != 7 * E:
        raise _invalid("measurements: one 7-vector per edge is needed")
    W = None
    if sqrt_information is not None:
        W = np.ascontiguousarray(sqrt_information, dtype=np.float64)
        if W.size != 49 * E:
            raise _invalid("sqrt_information: one 7 x 7 matrix per edge is needed")
    f = None
    if fixed is not None:
        f = np.ascontiguousarray(np.asarray(fixed).astype(bool), dtype=np.uint8).reshape(-1)
        if f.shape[0] != n:
            raise _invalid("fixed: one flag per node is needed")
    o = (options or Sim3PoseGraphOptions()).to_c()
    rows = max(int(o.max_num_iterations), 0) + 1 if want_trace else 0
    trace = np.zeros((rows, 5)) if want_trace else None
    summ = capi.PoseGraphSim3SummaryC()
    capi.check(capi.lib().theia_hip_pose_graph_sim3(n, capi.ptr(x, C.c_double), capi.ptr(f, C.c_uint8), E, capi.ptr(e, C.c_int32),
                                                    capi.ptr(z, C.c_double), capi.ptr(W, C.c_double), C.byref(o), C.byref(summ),
                                                    capi.ptr(trace, C.c_double), rows))
    return x, Sim3PoseGraphSummary(summ, trace[:summ.trace_size].copy() if want_trace else None)


def _rotations(cam_ext):
    from .synth import angle_axis_to_matrix
    return angle_axis_to_matrix(np.asarray(cam_ext, dtype=np.float64).reshape(-1, 6)[:, 3:6])


def Sim3sFromReconstruction(reconstruction):
    """GetSim3s (align_reconstructions_pose_graph_optim_test.cc:71-79) for every view, in view order:
    log(Sim3(RxSO3(1, R_c_w), -R_c_w C)) -> [num_views][7], through theia_hip_sim3_maps."""
    cams = np.asarray(reconstruction.cam_ext, dtype=np.float64).reshape(-1, 6)
    R = _rotations(cams)
    t = -np.einsum("nij,nj->ni", R, cams[:, :3])
    return sim3_maps(capi.THEIA_SIM3_MAP_LOG, np.concatenate([np.ones((len(cams), 1)), R.reshape(-1, 9), t], axis=1))


def _groups(nodes):
    o = sim3_maps(capi.THEIA_SIM3_MAP_TO_RTS, np.asarray(nodes, dtype=np.float64).reshape(-1, 7))
    return o[:, :9].reshape(-1, 3, 3), o[:, 9:12], o[:, 12]


def RelativeSim3s(nodes, edges):
    """log(exp(x_j) exp(x_i)^-1) per edge (i, j): the measurement that makes the edge's residual zero at `nodes` -> [E][7]."""
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    R, t, s = _groups(nodes)
    Ri, ti, si = R[e[:, 0]], t[e[:, 0]], s[e[:, 0]]
    Rj, tj, sj = R[e[:, 1]], t[e[:, 1]], s[e[:, 1]]
    Rr = np.einsum("nij,nkj->nik", Rj, Ri)                       # R_j R_i'
    sr = sj / si
    tr = tj - sr[:, None] * np.einsum("nij,nj->ni", Rr, ti)      # t_j - (s_j / s_i) R_j R_i' t_i
    return sim3_maps(capi.THEIA_SIM3_MAP_LOG, np.concatenate([sr[:, None], Rr.reshape(-1, 9), tr], axis=1))


def SetPosesFromSim3s(reconstruction, view_ids, nodes):
    """Writes nodes (tangents of camera-from-world similarities) back as poses: orientation from R, position -R' t / s."""
    from .synth import matrix_to_angle_axis
    ids = np.asarray(list(view_ids), dtype=np.int64)
    R, t, s = _groups(nodes)
    if len(ids) != len(s):
        raise _invalid("one node per view id is needed")
    cams = np.array(reconstruction.cam_ext, dtype=np.float64).reshape(-1, 6)
    cams[ids, :3] = -np.einsum("nji,nj->ni", R, t) / s[:, None]
    cams[ids, 3:6] = matrix_to_angle_axis(R)
    reconstruction.cam_ext = cams


def overlap_pose_graph(reconstruction1, reconstruction2, common_views=None, min_shared_tracks=1):
    """The graph AlignOverlapReconstructionsPoseGraph solves -> (nodes [n][7], fixed [n], edges [E][2], measurements [E][7],
    view_ids): nodes 0 .. len(view_ids) - 1 are reconstruction2's estimated views view_ids (free), the rest reconstruction1's
    common views (held); first the self edges of reconstruction2 (ViewGraphFromReconstruction, measured at its current poses),
    then one identity edge per common view that reconstruction2 has estimated."""
    from .covisibility import ViewGraphFromReconstruction
    r1, r2 = reconstruction1, reconstruction2
    common = FindCommonViewsByName(r1, r2) if common_views is None else list(common_views)
    id1 = {n: i for i, n in enumerate(_names(r1))}
    id2 = {n: i for i, n in enumerate(_names(r2))}
    view_ids = [v for v in range(r2.NumViews()) if r2.view_estimated[v]]
    local = {v: k for k, v in enumerate(view_ids)}
    x2, x1 = Sim3sFromReconstruction(r2), Sim3sFromReconstruction(r1)
    held = [n for n in common if id2[n] in local]
    nodes = np.concatenate([x2[view_ids], x1[[id1[n] for n in held]].reshape(-1, 7)])
    fixed = np.zeros(len(nodes), dtype=np.uint8)
    fixed[len(view_ids):] = 1
    self_edges = np.array([(local[a], local[b]) for (a, b) in ViewGraphFromReconstruction(r2, min_shared_tracks)
                           if a in local and b in local], dtype=np.int32).reshape(-1, 2)
    cross = np.array([(local[id2[n]], len(view_ids) + k) for k, n in enumerate(held)], dtype=np.int32).reshape(-1, 2)
    meas = np.concatenate([RelativeSim3s(nodes, self_edges) if len(self_edges) else np.zeros((0, 7)), np.zeros((len(cross), 7))])
    return nodes, fixed, np.concatenate([self_edges, cross]), meas, view_ids


def AlignOverlapReconstructionsPoseGraph(reconstruction1, reconstruction2, common_views=None, min_shared_tracks=1,
                                         cross_weight=1.0, options=None, want_trace=False):
    """The use align_reconstructions.h:61-68 declares and the reference never defines, from the pieces of
    pose_graph_sim3_error.h and align_reconstructions_pose_graph_optim.{h,cc}: reconstruction2's estimated views are free
    Sim(3) nodes, reconstruction1's common views (FindCommonViewsByName when not given) are held, an identity edge (weight
    cross_weight) ties each common pair, and reconstruction2's co-visibility graph (at least min_shared_tracks shared tracks)
    contributes self edges measured at its current poses, so that the correction the common views ask for is spread over the
    chunk instead of applied rigidly.  reconstruction2's poses are written back (positions -R' t / s); its TRACKS ARE LEFT
    ALONE: re-estimate them (EstimateAllTracks) or bundle-adjust afterwards.  Returns a Sim3PoseGraphSummary that also
    carries `nodes` (the graph's nodes after the solve, overlap_pose_graph's order) and `view_ids`."""
    nodes, fixed, edges, meas, view_ids = overlap_pose_graph(reconstruction1, reconstruction2, common_views, min_shared_tracks)
    if int(fixed.sum()) == 0:
        raise _invalid("the reconstructions have no estimated view in common")
    W = None
    if float(cross_weight) != 1.0:
        W = np.tile(np.eye(7), (len(edges), 1, 1))
        W[len(edges) - int(fixed.sum()):] *= float(cross_weight)
    out, summary = OptimizePoseGraphSim3(nodes, edges, meas, W, fixed, options, want_trace)
    SetPosesFromSim3s(reconstruction2, view_ids, out[:len(view_ids)])
    summary.nodes, summary.view_ids = out, view_ids   # the graph's nodes after the solve (the held ones last)
    return summary
