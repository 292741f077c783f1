"""GPU: the incremental-step stages on the device against the restatements of tests/incremental_ref.py.
Scores, counts and flags are compared by integer equality; the localisation by array equality with the same chain written
out in this file from the existing ransac.* and BundleAdjustView calls."""
import copy
import ctypes as C

import numpy as np
import pytest

from pytheiasfm_amd import _capi as capi, ba, incremental as inc, ransac, sfm, synth, twoview
from tests import fountain, incremental_ref as ref, incremental_scenes as scenes

pytestmark = pytest.mark.gpu
INVALID = capi.THEIA_HIP_ERR_INVALID_ARGUMENT


# ------------------------------------------------------------------ visibility scores
class Views:
    """Rows of theia_hip_visibility_scores built view by view."""

    def __init__(self, num_tracks):
        self.off, self.uv, self.tr, self.size = [0], [], [], []
        self.est = np.ones(num_tracks, np.uint8)

    def add(self, uv, tracks, size):
        uv = np.asarray(uv, dtype=np.float64).reshape(-1, 2)
        self.uv.extend(uv.tolist()); self.tr.extend(int(t) for t in tracks); self.size.append([int(size[0]), int(size[1])])
        self.off.append(len(self.tr))
        return self

    def device(self, levels=6):
        return inc.visibility_scores(self.off, np.array(self.uv).reshape(-1, 2), np.array(self.tr, np.int32), self.est,
                                     np.array(self.size, np.int32).reshape(-1, 2), levels)

    def restated(self, levels=6):
        n, s = [], []
        for v in range(len(self.size)):
            p = ref.VisibilityPyramid(self.size[v][0], self.size[v][1], levels)
            k = 0
            for row in range(self.off[v], self.off[v + 1]):
                if self.est[self.tr[row]]:
                    k += 1
                    p.add_point(self.uv[row][0], self.uv[row][1])
            n.append(k); s.append(p.compute_score())
        return n, s

    def check(self, levels=6):
        n, s = self.device(levels)
        rn, rs = self.restated(levels)
        assert n.tolist() == rn and s.tolist() == rs
        return n, s


def random_uv(rng, count, size):
    return rng.uniform(-0.1, 1.1, size=(count, 2)) * np.array(size, dtype=np.float64)


def test_scores_around_the_wave_and_workgroup_sizes():
    rng = np.random.default_rng(1)
    v = Views(2000)
    v.est[:] = rng.random(2000) < 0.7
    for count in (0, 1, 63, 64, 65, 257, 1025):
        v.add(random_uv(rng, count, (640, 480)), rng.choice(2000, size=count, replace=False), (640, 480))
    n, s = v.check()
    assert n[0] == 0 and s[0] == 0 and n[6] > 600


def _cut_reconstruction(estimated_counts, shared_uv=False):
    """One view per entry, 40 observations each of its own 40 tracks, the first `count` of them estimated."""
    rng = np.random.default_rng(2)
    nv = len(estimated_counts)
    r = sfm.Reconstruction()
    r.cam_ext = np.zeros((nv, 6)); r.view_estimated = np.zeros(nv, bool); r.points = np.zeros((40 * nv, 4))
    r.track_estimated = np.zeros(40 * nv, bool)
    r.obs_view = np.repeat(np.arange(nv), 40).astype(np.int32)
    r.obs_track = np.arange(40 * nv, dtype=np.int32)
    one = random_uv(rng, 40, (800, 600))
    r.obs_uv = np.vstack([one if shared_uv else random_uv(rng, 40, (800, 600)) for _ in range(nv)])
    for v, count in enumerate(estimated_counts):
        r.track_estimated[40 * v:40 * v + count] = True
    r.view_image_size = np.tile(np.array([800, 600], np.int32), (nv, 1))
    # interleave the rows: FindViewsToLocalize builds the by-view rows itself
    order = rng.permutation(len(r.obs_view))
    r.obs_view, r.obs_track, r.obs_uv = r.obs_view[order], r.obs_track[order], np.ascontiguousarray(r.obs_uv[order])
    return r


def _restated_find(r, views, **kw):
    return ref.find_views_to_localize(r.obs_view.tolist(), r.obs_track.tolist(), r.obs_uv.tolist(), r.track_estimated.tolist(),
                                      r.view_image_size.tolist(), list(views), **kw)


def test_find_views_applies_the_cut_at_30():
    r = _cut_reconstruction([29, 30, 31, 40, 0])
    got = inc.FindViewsToLocalize(r, range(5))
    assert sorted(got) == [1, 2, 3] and got == _restated_find(r, range(5))
    assert inc.FindViewsToLocalize(r, [0, 4]) == []
    assert inc.FindViewsToLocalize(r, range(5), min_num_observed_3d_points=29, num_pyramid_levels=3) == \
        _restated_find(r, range(5), min_points=29, levels=3)


def test_all_tracks_unestimated():
    rng = np.random.default_rng(3)
    v = Views(50)
    v.est[:] = 0
    v.add(random_uv(rng, 50, (640, 480)), range(50), (640, 480))
    n, s = v.check()
    assert n.tolist() == [0] and s.tolist() == [0]


@pytest.mark.parametrize("w", [640, 1000, 1])
def test_border_values(w):
    xs = [0.0, -0.0, -1e-300, np.nextafter(float(w), 0.0), float(w), 1e300, -1e300] + [w * k / 64 for k in range(65)]
    v = Views(1)
    for x in xs:                       # one view per value: x and y borders separately
        v.add([[x, 10.0]], [0], (w, 480))
        v.add([[10.0, x]], [0], (640, w))
    v.check()
    both = Views(1).add([[x, x] for x in xs], [0] * len(xs), (w, w))
    both.check()


def test_all_points_in_one_cell():
    rng = np.random.default_rng(4)
    uv = np.array([30.0, 22.5]) + rng.uniform(0.0, 7.0, size=(300, 2))      # cells of 10 x 7.5 pixels at six levels
    _, s = Views(1).add(uv, [0] * 300, (640, 480)).check()
    assert s.tolist() == [sum(4 ** (i + 1) for i in range(6))]


@pytest.mark.parametrize("levels", range(1, 7))
def test_every_finest_cell_exactly_once(levels):
    cells = 1 << levels
    uv = [[x + 0.5, 3 * y + 1.5] for x in range(cells) for y in range(cells)]
    _, s = Views(1).add(uv, [0] * len(uv), (cells, 3 * cells)).check(levels)
    assert s.tolist() == [sum(16 ** (i + 1) for i in range(levels))]


def test_levels_1_to_7_on_one_random_view():
    rng = np.random.default_rng(5)
    v = Views(1).add(random_uv(rng, 3000, (1920, 1080)), [0] * 3000, (1920, 1080))
    scores = [int(v.check(levels)[1][0]) for levels in range(1, 8)]
    assert scores == sorted(scores) and scores[0] == 16


def test_unequal_sides_and_a_width_of_one():
    rng = np.random.default_rng(6)
    v = Views(1)
    for size in ((4000, 30), (30, 4000), (1, 480), (640, 1), (1, 1), (2 ** 31 - 1, 7)):
        v.add(random_uv(rng, 200, size), [0] * 200, size)
    v.check()
    v.check(7)


def test_equal_scores_put_the_larger_id_first():
    r = _cut_reconstruction([40, 35, 40, 40], shared_uv=True)
    got = inc.FindViewsToLocalize(r, [0, 2, 3, 1])
    assert got == _restated_find(r, [0, 2, 3, 1])
    assert [g for g in got if g != 1] == [3, 2, 0]       # views 0, 2, 3 hold the same points


def test_200_random_views_in_one_call_and_the_same_bytes_twice():
    rng = np.random.default_rng(7)
    v = Views(5000)
    v.est[:] = rng.random(5000) < 0.5
    for _ in range(200):
        size = (int(rng.integers(1, 3000)), int(rng.integers(1, 3000)))
        count = int(rng.integers(0, 400))
        v.add(random_uv(rng, count, size), rng.choice(5000, size=count, replace=False), size)
    n1, s1 = v.check()
    n2, s2 = v.device()
    assert n1.tobytes() == n2.tobytes() and s1.tobytes() == s2.tobytes()


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_coordinate_is_refused_and_outputs_stay(bad):
    rng = np.random.default_rng(8)
    off = np.array([0, 100, 400], np.int64)
    uv = random_uv(rng, 400, (640, 480)); tr = np.arange(400, dtype=np.int32); est = np.ones(400, np.uint8)
    uv[333, 1] = bad
    est[333] = 0          # an observation of an unestimated track is still one of "the observations passed"
    size = np.array([[640, 480], [640, 480]], np.int32)
    n = np.full(2, -7, np.int32); s = np.full(2, -7, np.int32)
    rc = capi.lib().theia_hip_visibility_scores(2, capi.ptr(off, C.c_int64), capi.ptr(uv, C.c_double), capi.ptr(tr, C.c_int32), 400,
                                                capi.ptr(est, C.c_uint8), capi.ptr(size, C.c_int32), 6, capi.ptr(n, C.c_int32),
                                                capi.ptr(s, C.c_int32))
    assert rc == INVALID and (n == -7).all() and (s == -7).all()
    with pytest.raises(capi.TheiaHipError):
        inc.visibility_scores(off, uv, tr, est, size, 6)


def test_visibility_pyramid_object():
    rng = np.random.default_rng(9)
    p, q = inc.VisibilityPyramid(1920, 1080, 6), ref.VisibilityPyramid(1920, 1080, 6)
    assert p.ComputeScore() == 0
    for x, y in random_uv(rng, 500, (1920, 1080)):
        p.AddPoint((x, y)); q.add_point(x, y)
    assert p.ComputeScore() == q.compute_score()


# ------------------------------------------------------------------ underconstrained sweep
def _device_sweep(s):
    ve, te = s.view_estimated.copy(), s.track_estimated.copy()
    out = inc.set_underconstrained_unestimated(s.num_views, s.num_tracks, s.obs_view, s.obs_track, ve, te)
    return out, ve, te


@pytest.mark.parametrize("scene", [scenes.stopping_scene, scenes.cascade_scene, scenes.nothing_scene, scenes.everything_scene])
def test_sweep_on_hand_worked_scenes(scene):
    s = scene()
    out, ve, te = _device_sweep(s)
    assert out == s.expected[:3] and ve.tolist() == s.expected[3] and te.tolist() == s.expected[4]


@pytest.mark.parametrize("track_fraction", [0.5, 0.12])
def test_sweep_random_equals_the_restatement(track_fraction):
    s = scenes.random_sweep(track_fraction=track_fraction)
    rve, rte = s.view_estimated.astype(bool).tolist(), s.track_estimated.astype(bool).tolist()
    expected = ref.set_underconstrained_as_unestimated(s.obs_view.tolist(), s.obs_track.tolist(), rve, rte)
    out, ve, te = _device_sweep(s)
    assert out == expected and expected[1] > 0 and (track_fraction == 0.5 or (expected[0] > 0 and expected[2] > 2))
    assert ve.astype(bool).tolist() == rve and te.astype(bool).tolist() == rte
    # through the mirror, on a Reconstruction
    r = sfm.Reconstruction()
    r.cam_ext = np.zeros((s.num_views, 6)); r.points = np.zeros((s.num_tracks, 4))
    r.view_estimated, r.track_estimated = s.view_estimated.astype(bool), s.track_estimated.astype(bool)
    r.obs_view, r.obs_track = s.obs_view, s.obs_track
    assert inc.SetUnderconstrainedAsUnestimated(r) == expected
    assert r.view_estimated.tolist() == rve and r.track_estimated.tolist() == rte


def test_sweep_without_observations_clears_every_view_then_every_track():
    ve, te = np.ones(3, np.uint8), np.ones(2, np.uint8)
    assert inc.set_underconstrained_unestimated(3, 2, [], [], ve, te) == (3, 2, 2)
    assert not ve.any() and not te.any()


# ------------------------------------------------------------------ localisation
V = 2     # the unestimated view of scenes.localization_scene


def _options(**kw):
    o = inc.LocalizeViewToReconstructionOptions()
    o.ransac_params.min_iterations = 32
    o.ransac_params.max_iterations = 128
    o.ransac_params.seed = 11
    o.ba_options.max_num_iterations = 10
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _hand_matches(r, v, calibrated):
    """:77-123 element by element: the view's observations in order, estimated tracks only"""
    g = r.view_group[v]
    cam = ransac.Camera(r.cam_ext[v, :3], r.cam_ext[v, 3:6], r.group_intrinsics[g], r.group_model[g])
    rows = []
    for k in range(len(r.obs_view)):
        if r.obs_view[k] != v or not r.track_estimated[r.obs_track[k]]:
            continue
        X = r.points[r.obs_track[k]]
        if calibrated:
            f = cam.pixel_to_normalized(r.obs_uv[k])
        else:
            f = r.obs_uv[k] - np.array([r.group_intrinsics[g, 3], r.group_intrinsics[g, 4]])
        rows.append([f[0], f[1], X[0] / X[3], X[1] / X[3], X[2] / X[3]])
    return np.array(rows, dtype=np.float64).reshape(-1, 5)


def _hand_localize(r, v, o, branch):
    """The chain of LocalizeViewToReconstruction for a view that reaches its RANSAC call, from the existing entry points."""
    m = _hand_matches(r, v, branch != "p4pf")
    assert len(m) >= o.min_num_inliers
    w, h = r.view_image_size[v]
    thr = twoview.ComputeResolutionScaledThreshold(o.reprojection_error_threshold_pixels, int(w), int(h))
    rp = copy.copy(o.ransac_params)
    focal = r.group_intrinsics[r.view_group[v], 0]
    if branch == "known_orientation":
        rp.error_thresh = thr * thr / (focal * focal)
        ok, position, summary = ransac.EstimateAbsolutePoseWithKnownOrientation(rp, ransac.RansacType.RANSAC, r.cam_ext[v, 3:6], m)
        ok = ok and len(summary.inliers) > o.min_num_inliers
        if ok:
            r.cam_ext[v, :3] = position
    elif branch == "p4pf":
        rp.error_thresh = thr * thr
        ok, pose, summary = ransac.EstimateUncalibratedAbsolutePose(rp, ransac.RansacType.RANSAC, m)
        if ok:
            r.cam_ext[v, 3:6] = synth.matrix_to_angle_axis(pose.rotation)
            r.cam_ext[v, :3] = pose.position
            r.group_intrinsics[r.view_group[v], 0] = pose.focal_length
    else:
        rp.error_thresh = thr * thr / (focal * focal)
        ok, pose, summary = ransac.EstimateCalibratedAbsolutePose(rp, ransac.RansacType.RANSAC, branch, m)
        if ok:
            r.cam_ext[v, 3:6] = synth.matrix_to_angle_axis(pose.rotation)
            r.cam_ext[v, :3] = pose.position
    if not ok or len(summary.inliers) < o.min_num_inliers:
        return False, summary
    r.view_estimated[v] = True
    if o.bundle_adjust_view:
        return bool(sfm.BundleAdjustView(r, o.ba_options, v).success), summary
    return True, summary


def _same_state(a, b):
    for name in ("cam_ext", "group_intrinsics", "points", "view_estimated", "track_estimated"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name


def _same_summary(a, b):
    assert a.inliers == b.inliers and a.num_input_data_points == b.num_input_data_points
    assert a.num_iterations == b.num_iterations and a.confidence == b.confidence


def _displaced(r, v):
    """The view to localise starts away from its place, so that a pose that was not written shows."""
    r.cam_ext[v, :3] += np.array([0.7, -0.4, 0.3])
    return r


@pytest.mark.parametrize("bundle_adjust_view", [True, False])
@pytest.mark.parametrize("branch", [ransac.PnPType.KNEIP, ransac.PnPType.SQPnP, ransac.PnPType.DLS, "p4pf", "known_orientation"])
def test_localize_equals_the_hand_chain(branch, bundle_adjust_view):
    r = _displaced(scenes.localization_scene(), V)
    o = _options(bundle_adjust_view=bundle_adjust_view)
    if branch == "known_orientation":
        o.assume_known_orientation = True
    elif branch == "p4pf":
        r.group_intrinsics[0, 0] = 900.0      # a wrong focal length, to see it replaced
    else:
        o.pnp_type = branch
        r.view_focal_prior_set[V] = True
        r.cam_ext[V, 3:6] += 0.2
    hand = scenes.copy_reconstruction(r)
    start = scenes.copy_reconstruction(r)
    ok, summary = inc.LocalizeViewToReconstruction(V, o, r)
    hok, hsummary = _hand_localize(hand, V, o, branch)
    assert ok is True and hok is True
    _same_summary(summary, hsummary)
    _same_state(r, hand)
    assert r.view_estimated[V] and len(summary.inliers) >= o.min_num_inliers
    assert not np.array_equal(r.cam_ext[V], start.cam_ext[V])
    if branch == "p4pf":
        assert r.group_intrinsics[0, 0] != 900.0 and abs(r.group_intrinsics[0, 0] - 1000.0) < 50.0
    else:
        assert np.array_equal(r.group_intrinsics, start.group_intrinsics)
    if branch == "known_orientation" and not bundle_adjust_view:
        assert np.array_equal(r.cam_ext[V, 3:6], start.cam_ext[V, 3:6])


def test_too_few_inliers_leaves_the_view_unestimated():
    """45 matches, 20 of them moved 300 pixels away: the RANSAC succeeds with fewer than 30 inliers (:243).  The camera keeps
    the pose EstimateCameraPose wrote (:199-200), the view is not estimated and no BA runs."""
    r = _displaced(scenes.localization_scene(), V)
    r.view_focal_prior_set[V] = True
    rows = np.flatnonzero(r.obs_view == V)
    r.track_estimated[r.obs_track[rows[45:]]] = False
    r.obs_uv[rows[:20]] += 300.0
    o = _options(pnp_type=ransac.PnPType.KNEIP)
    hand = scenes.copy_reconstruction(r)
    ok, summary = inc.LocalizeViewToReconstruction(V, o, r)
    hok, hsummary = _hand_localize(hand, V, o, ransac.PnPType.KNEIP)
    assert ok is False and hok is False and summary.num_input_data_points == 45
    assert len(summary.inliers) < o.min_num_inliers
    _same_summary(summary, hsummary)
    _same_state(r, hand)
    assert not r.view_estimated[V]


def test_known_orientation_needs_strictly_more_than_min_num_inliers():
    """An outlier-free scene with exactly 30 matches: all 30 are inliers (the hand chain's RANSAC call shows it), which
    passes `>= 30` (:243) but not the branch's own `> 30` (:177): the view is not localised and its position is not written.
    With min_num_inliers = 29 the same data localise it."""
    r = _displaced(scenes.localization_scene(pixel_noise=0.0), V)
    rows = np.flatnonzero(r.obs_view == V)
    r.track_estimated[r.obs_track[rows[30:]]] = False
    o = _options(assume_known_orientation=True, bundle_adjust_view=False)
    m = _hand_matches(r, V, True)
    assert len(m) == 30
    rp = copy.copy(o.ransac_params)
    thr = twoview.ComputeResolutionScaledThreshold(4.0, *scenes.IMAGE_SIZE)
    rp.error_thresh = thr * thr / r.group_intrinsics[0, 0] ** 2
    hok, _, hsummary = ransac.EstimateAbsolutePoseWithKnownOrientation(rp, ransac.RansacType.RANSAC, r.cam_ext[V, 3:6], m)
    assert hok and len(hsummary.inliers) == 30
    start = scenes.copy_reconstruction(r)
    ok, summary = inc.LocalizeViewToReconstruction(V, o, r)
    assert ok is False and len(summary.inliers) == 30
    _same_state(r, start)
    o.min_num_inliers = 29
    ok, summary = inc.LocalizeViewToReconstruction(V, o, r)
    assert ok is True and len(summary.inliers) == 30 and r.view_estimated[V]
    assert np.abs(r.cam_ext[V, :3] - (start.cam_ext[V, :3] - np.array([0.7, -0.4, 0.3]))).max() < 1e-6


def _three_view_scene():
    r = scenes.localization_scene(seed=0x10CA3, num_views=8, num_tracks=260, num_groups=2, unestimated_view=None)
    for v in (1, 3, 6):
        r.view_estimated[v] = False
        _displaced(r, v)
    r.view_focal_prior_set[[1, 3]] = True       # views 1, 3: calibrated (one merged call); view 6: P4Pf
    return r


@pytest.mark.parametrize("use_rng", [False, True])
def test_localize_views_equals_the_loop(use_rng):
    o = _options()
    views = [1, 3, 6]
    a, b = _three_view_scene(), _three_view_scene()
    state = ransac.RandomNumberGenerator.thread_state()
    if use_rng:
        o.ransac_params.rng = ransac.RandomNumberGenerator(5)
    before = bytes(state)          # the whole theia_rng_state, its DLS / P4Pfr counters included
    loop = [inc.LocalizeViewToReconstruction(v, o, a) for v in views]
    after_loop = bytes(state)
    C.memmove(C.addressof(state), before, len(before))
    batch = inc.LocalizeViewsToReconstruction(views, o, b)
    assert [x[0] for x in loop] == [True, True, True] == [x[0] for x in batch]
    for (_, s1), (_, s2) in zip(loop, batch):
        _same_summary(s1, s2)
    _same_state(a, b)
    assert bytes(state) == after_loop
    if use_rng:
        assert after_loop != before


# ------------------------------------------------------------------ one round, end to end
def _rays(d, cam_ext, obs_cam, obs_uv):
    f, a, s, px, py, _, _ = d["intrinsics"][0]
    y = (obs_uv[:, 1] - py) / (f * a)
    x = (obs_uv[:, 0] - px - s * y) / f
    R = synth.angle_axis_to_matrix(cam_ext[:, 3:6])
    ray = np.einsum("nji,nj->ni", R[obs_cam], np.column_stack([x, y, np.ones(len(x))]))
    return ray / np.linalg.norm(ray, axis=1, keepdims=True)


def test_one_round_on_fountain():
    """score -> localise -> remove outliers -> triangulate -> BA -> sweep on fountain-P11, with view 7 and the tracks only it
    and one other view see un-estimated.  Asserted: what the rules guarantee."""
    d = fountain.load()
    v = 7
    r = sfm.Reconstruction.from_flat(fountain.flat_problem(d))
    # the file carries an image size for one view only (zeros elsewhere); the Strecha fountain-P11 images are 3072 x 2048
    size = d["image_size"].astype(np.int32)
    r.view_image_size = np.where(size.any(axis=1)[:, None], size, np.array([3072, 2048], np.int32)).astype(np.int32)
    r.view_focal_prior_set = np.zeros(r.NumViews(), bool)
    r.view_focal_prior_set[v] = True
    length = np.bincount(r.obs_track, minlength=r.NumTracks())
    in_v = np.zeros(r.NumTracks(), bool)
    in_v[r.obs_track[r.obs_view == v]] = True
    r.view_estimated[v] = False
    r.track_estimated[in_v & (length == 2)] = False
    _displaced(r, v)

    assert inc.FindViewsToLocalize(r, [v]) == [v]
    o = _options()
    ok, summary = inc.LocalizeViewToReconstruction(v, o, r)
    assert ok and r.view_estimated[v] and len(summary.inliers) >= o.min_num_inliers

    tracks_of_v = np.flatnonzero(in_v)
    sfm.SetOutlierTracksToUnestimated(tracks_of_v.tolist(), 5.0, 3.0, r)
    # theia_hip_estimate_tracks on the tracks of the view over the estimated views: the estimated ones are constant points,
    # which the entry leaves alone.  (Every track of this file has three or more views, so un-estimating "the tracks only
    # this and one other view see" takes none away: what is left to triangulate is what the outlier sweep removed.)
    const = r.track_estimated[tracks_of_v].copy()
    local = -np.ones(r.NumTracks(), np.int64); local[tracks_of_v] = np.arange(len(tracks_of_v))
    keep = (local[r.obs_track] >= 0) & r.view_estimated[r.obs_view]
    flat = capi.FlatProblem(r.cam_ext.copy(), r.group_intrinsics.copy(), r.group_model, r.view_group, r.points[tracks_of_v].copy(),
                            r.obs_uv[keep], r.obs_view[keep], local[r.obs_track[keep]].astype(np.int32),
                            point_const=const.astype(np.uint8))
    bo = sfm.BundleAdjustmentOptions(); bo.max_num_iterations = 10; bo.use_inner_iterations = False
    est, _ = ba.estimate_tracks(flat, _rays(d, r.cam_ext, r.obs_view[keep], r.obs_uv[keep]), bo.to_c(), 3.0, 5.0, True)
    new = est & ~const
    r.points[tracks_of_v[new]] = flat.points[new]
    r.track_estimated[tracks_of_v[new]] = True
    assert np.array_equal(flat.points[const], r.points[tracks_of_v[const]])
    sfm.BundleAdjustPartialReconstruction(bo, [v], tracks_of_v[r.track_estimated[tracks_of_v]].tolist(), r)

    rve, rte = r.view_estimated.tolist(), r.track_estimated.tolist()
    expected = ref.set_underconstrained_as_unestimated(r.obs_view.tolist(), r.obs_track.tolist(), rve, rte)
    assert inc.SetUnderconstrainedAsUnestimated(r) == expected
    assert r.view_estimated.tolist() == rve and r.track_estimated.tolist() == rte
    assert r.view_estimated[v]
