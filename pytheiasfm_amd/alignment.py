"""Host-side mirror of pyTheia's reconstruction alignment (src/theia/sfm/transformation/, exported in
src/pytheia/sfm/sfm.cc:620-628,938) over theia_hip_align_point_clouds, theia_hip_transform_reconstruction and the RANSAC
estimator THEIA_EST_CAMERA_ALIGNMENT (include/theia_hip.h).

Same names as the pybind wrappers; the Align* functions return (rotation [3][3], translation [3], scale).  Reconstructions are
the array-backed pytheiasfm_amd.sfm.Reconstruction; the functions that match views by name need its `view_names`.
Not built: OptimizeAlignmentSim3 and the Sim3 conversions, align_reconstructions_pose_graph_optim."""
import ctypes as C

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
