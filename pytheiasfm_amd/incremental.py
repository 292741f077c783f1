"""The stages of the incremental estimator's inner loop that join the absolute-pose RANSACs, the track estimator and the
bundle adjustments (sfm/incremental_reconstruction_estimator.cc; the hybrid estimator repeats the same loop):

    score (FindViewsToLocalize) -> localise (LocalizeViewToReconstruction) -> remove outliers -> triangulate -> BA ->
    sweep (SetUnderconstrainedAsUnestimated)

The visibility scores and the underconstrained sweep run on the device (csrc/next_view.hip); the localisation is a literal
restatement of sfm/localize_view_to_reconstruction.cc:54-262 on the existing `ransac.Estimate*` and `sfm.BundleAdjustView`
calls.  The estimator object, BuildTracksIncremental and ChooseInitialViewPair's trial loop are not built.

`sfm.Reconstruction` carries two optional fields for these stages: `view_image_size` ([nv][2] width, height) and
`view_focal_prior_set` ([nv] bool: View::CameraIntrinsicsPrior().focal_length.is_set; None = all false).
"""
import copy
import ctypes as C

import numpy as np

from . import _capi as capi
from . import ransac as _ransac
from . import sfm as _sfm
from . import synth as _synth
from .twoview import ComputeResolutionScaledThreshold

kMinNumObserved3dPoints = 30   # incremental_reconstruction_estimator.cc:426
kNumPyramidLevels = 6          # :427


def _invalid(message):
    return capi.TheiaHipError(capi.THEIA_HIP_ERR_INVALID_ARGUMENT, message)


def _image_sizes(reconstruction):
    size = reconstruction.view_image_size
    if size is None:
        raise _invalid("the reconstruction carries no view_image_size")
    size = np.ascontiguousarray(size, dtype=np.int32).reshape(-1, 2)
    if size.shape[0] != reconstruction.NumViews():
        raise _invalid("view_image_size must hold one (width, height) per view")
    return size


def visibility_scores(obs_off, obs_uv, obs_track, track_estimated, image_size, num_pyramid_levels):
    """theia_hip_visibility_scores -> (num_estimated_tracks [nv], score [nv]); the arrays as the C-ABI takes them."""
    obs_off = np.ascontiguousarray(obs_off, dtype=np.int64).reshape(-1)
    nv = len(obs_off) - 1
    uv = np.ascontiguousarray(obs_uv, dtype=np.float64).reshape(-1, 2)
    tr = np.ascontiguousarray(obs_track, dtype=np.int32).reshape(-1)
    est = np.ascontiguousarray(track_estimated, dtype=np.uint8).reshape(-1)
    size = np.ascontiguousarray(image_size, dtype=np.int32).reshape(-1, 2)
    nt = len(est)
    if size.shape[0] != nv or len(tr) != len(uv):
        raise _invalid("image_size holds one row per view, obs_uv one per obs_track")
    if nv > 0 and int(obs_off[-1]) > len(tr):
        raise _invalid("obs_off runs past the observations")
    # an empty numpy array may hand over a NULL pointer: the entry refuses that, so pad (the pad is never read)
    pad = lambda a, shape: a if a.size else np.zeros(shape, dtype=a.dtype)
    uv, tr, est = pad(uv, (1, 2)), pad(tr, 1), pad(est, 1)
    n_est = np.zeros(max(nv, 1), dtype=np.int32)
    score = np.zeros(max(nv, 1), dtype=np.int32)
    capi.check(capi.lib().theia_hip_visibility_scores(
        nv, capi.ptr(obs_off, C.c_int64), capi.ptr(uv, C.c_double), capi.ptr(tr, C.c_int32), nt, capi.ptr(est, C.c_uint8),
        capi.ptr(pad(size, (1, 2)), C.c_int32), int(num_pyramid_levels), capi.ptr(n_est, C.c_int32), capi.ptr(score, C.c_int32)))
    return n_est[:nv], score[:nv]


class VisibilityPyramid:
    """sfm/visibility_pyramid.h for a caller that holds one view: the same device call on one row."""

    def __init__(self, width, height, num_pyramid_levels):
        if int(width) <= 0 or int(height) <= 0 or int(num_pyramid_levels) <= 0:   # CHECK_GT (visibility_pyramid.cc:54-56)
            raise _invalid("VisibilityPyramid: width, height and num_pyramid_levels must be positive")
        self.width, self.height, self.num_pyramid_levels = int(width), int(height), int(num_pyramid_levels)
        self._points = []

    def AddPoint(self, point):
        self._points.append((float(point[0]), float(point[1])))

    def ComputeScore(self):
        n = len(self._points)
        _, score = visibility_scores([0, n], np.asarray(self._points, dtype=np.float64).reshape(n, 2), np.zeros(n, np.int32),
                                     np.ones(1, np.uint8), [[self.width, self.height]], self.num_pyramid_levels)
        return int(score[0])


def _rows_by_view(reconstruction, view_ids):
    """The by-view CSR of the listed views: (offsets [n + 1], observation rows), a view's rows in array order (stable sort)."""
    r = reconstruction
    order = np.argsort(r.obs_view, kind="stable")
    bounds = np.searchsorted(r.obs_view[order], np.arange(r.NumViews() + 1))
    count = bounds[view_ids + 1] - bounds[view_ids]
    off = np.zeros(len(view_ids) + 1, dtype=np.int64)
    off[1:] = np.cumsum(count)
    within = np.arange(int(off[-1]), dtype=np.int64) - np.repeat(off[:-1], count)
    return off, order[np.repeat(bounds[view_ids], count) + within]


def FindViewsToLocalize(reconstruction, unlocalized_views, min_num_observed_3d_points=kMinNumObserved3dPoints,
                        num_pyramid_levels=kNumPyramidLevels):
    """incremental_reconstruction_estimator.cc:422-463: the unlocalised views that observe at least
    `min_num_observed_3d_points` estimated tracks, sorted by (visibility score, view id) descending (std::greater on the
    pair: among equal scores the larger id first)."""
    r = reconstruction
    size = _image_sizes(r)
    ids = _sfm._ids(unlocalized_views)
    if len(ids) and (ids.min() < 0 or ids.max() >= r.NumViews()):
        raise _invalid("view id out of range (reference: CHECK_NOTNULL aborts)")
    if not len(ids):
        return []
    off, rows = _rows_by_view(r, ids)
    n_est, score = visibility_scores(off, r.obs_uv[rows], r.obs_track[rows], r.track_estimated, size[ids], num_pyramid_levels)
    keep = n_est >= int(min_num_observed_3d_points)
    return [int(v) for _, v in sorted(zip(score[keep].tolist(), ids[keep].tolist()), reverse=True)]


def _estimated_tracks_per_view(r):
    return np.bincount(r.obs_view[r.track_estimated[r.obs_track]], minlength=r.NumViews())


def _estimated_views_per_track(r):
    return np.bincount(r.obs_track[r.view_estimated[r.obs_view]], minlength=r.NumTracks())


def SetUnderconstrainedTracksToUnestimated(reconstruction):
    """reconstruction_estimator_utils.cc:291-319: estimated tracks seen by fewer than 2 estimated views; returns how many."""
    r = reconstruction
    gone = r.track_estimated & (_estimated_views_per_track(r) < 2)
    r.track_estimated[gone] = False
    return int(gone.sum())


def SetUnderconstrainedViewsToUnestimated(reconstruction):
    """reconstruction_estimator_utils.cc:321-350: estimated views that see fewer than 3 estimated tracks; returns how many."""
    r = reconstruction
    gone = r.view_estimated & (_estimated_tracks_per_view(r) < 3)
    r.view_estimated[gone] = False
    return int(gone.sum())


def set_underconstrained_unestimated(num_views, num_tracks, obs_view, obs_track, view_estimated, track_estimated):
    """theia_hip_set_underconstrained_unestimated on uint8 flag arrays, updated in place -> (views_removed, tracks_removed, rounds)."""
    ov = np.ascontiguousarray(obs_view, dtype=np.int32).reshape(-1)
    ot = np.ascontiguousarray(obs_track, dtype=np.int32).reshape(-1)
    if len(ov) != len(ot) or len(view_estimated) != num_views or len(track_estimated) != num_tracks:
        raise _invalid("one obs_view per obs_track, one flag per view and per track")
    for a in (view_estimated, track_estimated):
        if a.dtype != np.uint8 or not a.flags["C_CONTIGUOUS"]:
            raise _invalid("the flag arrays are contiguous uint8")
    nv_gone, nt_gone, rounds = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    capi.check(capi.lib().theia_hip_set_underconstrained_unestimated(
        int(num_views), int(num_tracks), len(ov), capi.ptr(ov if len(ov) else None, C.c_int32),
        capi.ptr(ot if len(ot) else None, C.c_int32), capi.ptr(view_estimated if num_views else None, C.c_uint8),
        capi.ptr(track_estimated if num_tracks else None, C.c_uint8),
        C.byref(nv_gone), C.byref(nt_gone), C.byref(rounds)))
    return nv_gone.value, nt_gone.value, rounds.value


def SetUnderconstrainedAsUnestimated(reconstruction):
    """The estimators' loop (incremental_reconstruction_estimator.cc:612-620, global_reconstruction_estimator.cc:100-110) on the
    device: view pass, track pass, while BOTH removed something.  Returns (views removed, tracks removed, rounds)."""
    r = reconstruction
    ve = r.view_estimated.astype(np.uint8)
    te = r.track_estimated.astype(np.uint8)
    out = set_underconstrained_unestimated(r.NumViews(), r.NumTracks(), r.obs_view, r.obs_track, ve, te)
    r.view_estimated[:] = ve != 0
    r.track_estimated[:] = te != 0
    return out


def NumEstimatedViews(reconstruction):
    return int(np.count_nonzero(reconstruction.view_estimated))


def NumEstimatedTracks(reconstruction):
    return int(np.count_nonzero(reconstruction.track_estimated))


def OrderViewPairsByInitializationCriterion(view_pairs, min_num_verified_matches):
    """incremental_reconstruction_estimator.cc:384-420.  view_pairs: {(id1, id2): TwoViewInfo} (or its items).  Keeps the pairs
    with num_verified_matches > min and sorts by (num_homography_inliers, -num_verified_matches, (id1, id2)) ascending."""
    items = view_pairs.items() if hasattr(view_pairs, "items") else view_pairs
    crit = [(int(info.num_homography_inliers), -int(info.num_verified_matches), (int(pair[0]), int(pair[1])))
            for pair, info in items if info.num_verified_matches > min_num_verified_matches]
    crit.sort()
    return [c[2] for c in crit]


class LocalizeViewToReconstructionOptions:
    """localize_view_to_reconstruction.h:50-79, same fields and defaults."""

    def __init__(self):
        self.reprojection_error_threshold_pixels = 4.0
        self.assume_known_orientation = False
        self.ransac_params = _ransac.RansacParameters()
        self.bundle_adjust_view = True
        self.ba_options = _sfm.BundleAdjustmentOptions()
        self.min_num_inliers = 30
        self.pnp_type = _ransac.PnPType.DLS


def _focal_prior_set(r, view_id):
    return r.view_focal_prior_set is not None and bool(r.view_focal_prior_set[view_id])


def DoesViewHaveKnownIntrinsics(reconstruction, view_id):
    """localize_view_to_reconstruction.cc:54-75, as written: the inner loop re-reads the view being localised (:69), so
    without a focal-length prior the answer is "this view is estimated and shares its intrinsics with another view"."""
    r = reconstruction
    if _focal_prior_set(r, view_id):
        return True
    group = r.view_group[view_id]
    for shared in np.flatnonzero(r.view_group == group):
        view = view_id                      # :69  const View* view = reconstruction.View(view_id);
        if r.view_estimated[view] and view_id != shared:
            return True
    return False


_BRANCH_KNOWN_ORIENTATION, _BRANCH_CALIBRATED, _BRANCH_UNCALIBRATED = range(3)


class _Prepared:
    """One view up to its RANSAC call: the branch, the 2D-3D matches (:77-123) and the scaled threshold (:147-208)."""
    pass


def _prepare(view_id, options, r, normalized_features):
    p = _Prepared()
    p.view_id = view_id
    known_intrinsics = bool(options.assume_known_orientation) or DoesViewHaveKnownIntrinsics(r, view_id)   # :235-237
    rows = np.flatnonzero(r.obs_view == view_id)
    rows = rows[r.track_estimated[r.obs_track[rows]]]
    group = r.view_group[view_id]
    intr = r.group_intrinsics[group]
    if known_intrinsics:
        if normalized_features is not None:
            feat = np.asarray(normalized_features, dtype=np.float64).reshape(-1, 2)[rows]
        else:    # pinhole only: ransac.Camera.pixel_to_normalized raises THEIA_HIP_ERR_UNSUPPORTED for the other models
            cam = _ransac.Camera(r.cam_ext[view_id, :3], r.cam_ext[view_id, 3:6], intr, r.group_model[group])
            feat = np.array([cam.pixel_to_normalized(uv) for uv in r.obs_uv[rows]], dtype=np.float64).reshape(-1, 2)
    else:
        feat = r.obs_uv[rows] - intr[3:5]
    X = r.points[r.obs_track[rows]]
    p.matches = np.ascontiguousarray(np.column_stack([feat, X[:, :3] / X[:, 3:4]]))
    p.branch = None
    if len(p.matches) < options.min_num_inliers:      # :141-145, before any device work
        return p
    size = _image_sizes(r)[view_id]
    thr = ComputeResolutionScaledThreshold(options.reprojection_error_threshold_pixels, int(size[0]), int(size[1]))
    p.params = copy.copy(options.ransac_params)
    focal = float(intr[0])
    if options.assume_known_orientation:
        p.branch = _BRANCH_KNOWN_ORIENTATION
        p.params.error_thresh = thr * thr / (focal * focal)
    elif known_intrinsics:
        p.branch = _BRANCH_CALIBRATED
        p.params.error_thresh = thr * thr / (focal * focal)
    else:
        p.branch = _BRANCH_UNCALIBRATED
        p.params.error_thresh = thr * thr
    return p


def _estimate(p, options, r):
    """The RANSAC call of the view's branch through the ransac.Estimate* wrappers -> (success, model, summary)."""
    RANSAC = _ransac.RansacType.RANSAC
    if p.branch == _BRANCH_KNOWN_ORIENTATION:
        return _ransac.EstimateAbsolutePoseWithKnownOrientation(p.params, RANSAC, r.cam_ext[p.view_id, 3:6], p.matches)
    if p.branch == _BRANCH_CALIBRATED:
        return _ransac.EstimateCalibratedAbsolutePose(p.params, RANSAC, options.pnp_type, p.matches)
    return _ransac.EstimateUncalibratedAbsolutePose(p.params, RANSAC, p.matches)


def _finish(p, ok, model, summary, options, r):
    """:160-221 after the RANSAC call, then :243-261."""
    v = p.view_id
    if p.branch == _BRANCH_KNOWN_ORIENTATION:
        # strict `>` (:177); never falls through to P3P (:180-182)
        success = bool(ok) and len(summary.inliers) > options.min_num_inliers
        if success:
            r.cam_ext[v, :3] = model
    else:
        success = bool(ok)
        if success:
            r.cam_ext[v, 3:6] = _synth.matrix_to_angle_axis(model.rotation)
            r.cam_ext[v, :3] = model.position
            if p.branch == _BRANCH_UNCALIBRATED:
                r.group_intrinsics[r.view_group[v], 0] = model.focal_length     # Camera::SetFocalLength: the shared intrinsics
    if not success or len(summary.inliers) < options.min_num_inliers:           # :243
        return False
    r.view_estimated[v] = True
    if options.bundle_adjust_view:
        return bool(_sfm.BundleAdjustView(r, options.ba_options, v).success)
    return True


def LocalizeViewToReconstruction(view_id, options, reconstruction, normalized_features=None):
    """localize_view_to_reconstruction.cc:225-262 -> (success, RansacSummary).  normalized_features (optional, one row per row of
    reconstruction.obs_uv): Camera::PixelToNormalizedCoordinates(pixel).hnormalized() of every observation, for the camera
    models whose un-projection the mirror does not restate (every model but the pinhole)."""
    r = reconstruction
    view_id = int(view_id)
    if view_id < 0 or view_id >= r.NumViews():
        raise _invalid("view id out of range (reference: CHECK_NOTNULL aborts)")
    p = _prepare(view_id, options, r, normalized_features)
    if p.branch is None:
        return False, _ransac.RansacSummary()
    ok, model, summary = _estimate(p, options, r)
    return _finish(p, ok, model, summary, options, r), summary


def _estimate_run(run, options, r):
    """The RANSAC calls of consecutive views of one branch as one estimate_batch call: every problem on the parameters' seed, or,
    with ransac_params.rng, as successive calls on the calling thread's generator.  Problem for problem what _estimate returns."""
    branch = run[0].branch
    if branch == _BRANCH_KNOWN_ORIENTATION:
        est = _ransac.EST_ABSOLUTE_POSE_KNOWN_ORIENTATION
        data = [_ransac.RotateCorrespondences(p.matches, r.cam_ext[p.view_id, 3:6]) for p in run]
    elif branch == _BRANCH_CALIBRATED:
        est = {_ransac.PnPType.KNEIP: _ransac.EST_ABS_KNEIP, _ransac.PnPType.DLS: _ransac.EST_ABS_DLS,
               _ransac.PnPType.SQPnP: _ransac.EST_ABS_SQPNP}[_ransac.PnPType(options.pnp_type)]
        data = [p.matches for p in run]
    else:
        est = _ransac.EST_UNCALIBRATED_ABSOLUTE_POSE
        data = [p.matches for p in run]
    off = np.zeros(len(run) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(d) for d in data])
    out = []
    # the threshold is per view (image size, focal length): views of one threshold share a call
    k = 0
    while k < len(run):
        e = k + 1
        while e < len(run) and run[e].params.error_thresh == run[k].params.error_thresh:
            e += 1
        pc = run[k].params.to_c()
        pc.ransac_type = int(_ransac.RansacType.RANSAC)
        sub = off[k:e + 1] - off[k]
        rows = np.vstack(data[k:e])
        if options.ransac_params.rng is None:
            res = _ransac.estimate_batch(est, rows, sub, pc, seeds=np.full(e - k, int(pc.seed), dtype=np.int64))
        else:
            res = _ransac.estimate_batch(est, rows, sub, pc, streams=(_ransac.RandomNumberGenerator.thread_state(), None))
        for i in range(e - k):
            s = _ransac.RansacSummary()
            s.inliers = np.nonzero(res["inlier_mask"][sub[i]:sub[i + 1]])[0].tolist()
            s.num_input_data_points = int(sub[i + 1] - sub[i])
            s.num_iterations = int(res["num_iterations"][i])
            s.confidence = float(res["confidence"][i])
            s.num_lo_iterations = int(res["num_lo_iterations"][i])
            m = res["models"][i]
            if branch == _BRANCH_KNOWN_ORIENTATION:
                model = m[0:3].copy()
            elif branch == _BRANCH_CALIBRATED:
                model = _ransac.CalibratedAbsolutePose(m)
            else:    # EstimateUncalibratedAbsolutePose (ransac.py) after its RANSAC call
                good, K, aa, position = _ransac.DecomposeProjectionMatrix(m[:12])
                model = _ransac.UncalibratedAbsolutePose(_synth.angle_axis_to_matrix(aa[None])[0], position,
                                                         K[0, 0] / K[2, 2] if good else 0.0)
            out.append((bool(res["success"][i]), model, s))
        k = e
    return out


def LocalizeViewsToReconstruction(view_ids, options, reconstruction, normalized_features=None):
    """[LocalizeViewToReconstruction(v, options, reconstruction) for v in view_ids], bit for bit, with the RANSAC calls of
    consecutive views that take the same branch merged into one estimate_batch call.  An extension: the reference localises
    one view per call.  The merge needs the views of a run not to read what an earlier one of the run writes.  A view writes
    its own pose and flag, in the P4Pf branch its group's focal length (which the P4Pf branch does not read), and its
    BundleAdjustView whatever intrinsics_to_optimize frees; so with intrinsics freed, with a view listed twice, or with a
    problem smaller than the minimal sample (which the single call refuses) this is the plain loop.  The view BAs stay
    single BundleAdjustView calls: BundleAdjustViewsIndependently is a different solver path and does not give the same bits."""
    r = reconstruction
    ids = [int(v) for v in view_ids]
    for v in ids:
        if v < 0 or v >= r.NumViews():
            raise _invalid("view id out of range (reference: CHECK_NOTNULL aborts)")
    loop = (len(set(ids)) != len(ids) or
            (options.bundle_adjust_view and int(options.ba_options.intrinsics_to_optimize) != 0))
    results = []
    k = 0
    while k < len(ids):
        p = _prepare(ids[k], options, r, normalized_features)
        if p.branch is None:
            results.append((False, _ransac.RansacSummary()))
            k += 1
            continue
        run = [p]
        if not loop:
            # the views behind it that take the same branch (a view with too few matches makes no RANSAC call: it stays in
            # the run and returns False in its place)
            while k + len(run) < len(ids):
                q = _prepare(ids[k + len(run)], options, r, normalized_features)
                if q.branch is not None and q.branch != p.branch:
                    break
                run.append(q)
        live = [q for q in run if q.branch is not None]
        sample = {_BRANCH_KNOWN_ORIENTATION: 2, _BRANCH_CALIBRATED: 3, _BRANCH_UNCALIBRATED: 4}[p.branch]
        if len(live) == 1 or any(len(q.matches) < sample for q in live):
            run = [p]
            estimates = [_estimate(p, options, r)]
        else:
            estimates = _estimate_run(live, options, r)
        it = iter(estimates)
        for q in run:
            if q.branch is None:
                results.append((False, _ransac.RansacSummary()))
                continue
            ok, model, summary = next(it)
            results.append((_finish(q, ok, model, summary, options, r), summary))
        k += len(run)
    return results
