"""CPU: the incremental-step stages.  The restatements of tests/incremental_ref.py against answers worked out
by hand, the host side of pytheiasfm_amd/incremental.py, and every refusal of theia_hip_visibility_scores /
theia_hip_set_underconstrained_unestimated that returns before a device is touched.  The device code is tested in
tests/test_incremental_step_gpu.py."""
import ctypes as C

import numpy as np
import pytest

from pytheiasfm_amd import _capi as capi, incremental as inc, ransac, sfm, twoview
import pytheiasfm_amd
from tests import incremental_ref as ref, incremental_scenes as scenes

INVALID = capi.THEIA_HIP_ERR_INVALID_ARGUMENT


# ------------------------------------------------------------------ the restatement against hand-worked answers
def test_empty_pyramid_scores_zero():
    assert ref.VisibilityPyramid(640, 480, 6).compute_score() == 0


@pytest.mark.parametrize("levels", range(1, 8))
def test_one_point_scores_one_cell_per_level(levels):
    p = ref.VisibilityPyramid(640, 480, levels)
    p.add_point(100.5, 17.25)
    assert p.compute_score() == sum(4 ** (i + 1) for i in range(levels))


@pytest.mark.parametrize("levels", range(1, 7))
def test_every_finest_cell_once_scores_full_levels(levels):
    cells = 1 << levels
    p = ref.VisibilityPyramid(cells, 3 * cells, levels)
    for x in range(cells):
        for y in range(cells):
            p.add_point(x + 0.5, 3 * y + 1.5)
    assert p.compute_score() == sum(16 ** (i + 1) for i in range(levels))


def test_border_cells_of_the_restatement():
    p = ref.VisibilityPyramid(640, 480, 6)
    for x, cell in ((0.0, 0), (-0.0, 0), (-1e-300, 0), (-5.0, 0), (10.0, 1), (9.999, 0), (np.nextafter(640.0, 0.0), 63), (640.0, 63),
                    (1e300, 63), (-1e300, 0)):
        assert ref.clamp(int(p.max_cells * float(x) / p.width), 0, p.max_cells - 1) == cell, x


@pytest.mark.parametrize("scene", [scenes.stopping_scene, scenes.cascade_scene, scenes.nothing_scene, scenes.everything_scene])
def test_restated_sweep_on_hand_worked_scenes(scene):
    s = scene()
    ve, te = s.view_estimated.astype(bool).tolist(), s.track_estimated.astype(bool).tolist()
    out = ref.set_underconstrained_as_unestimated(s.obs_view.tolist(), s.obs_track.tolist(), ve, te)
    assert out == s.expected[:3]
    assert [int(f) for f in ve] == s.expected[3] and [int(f) for f in te] == s.expected[4]


def test_restated_single_passes_agree_with_the_bucketed_loop():
    s = scenes.cascade_scene()
    ov, ot = s.obs_view.tolist(), s.obs_track.tolist()
    ve, te = [True] * s.num_views, [True] * s.num_tracks
    assert ref.set_underconstrained_views(ov, ot, ve, te) == 1 and ref.set_underconstrained_tracks(ov, ot, ve, te) == 2
    assert ref.set_underconstrained_views(ov, ot, ve, te) == 1 and ref.set_underconstrained_tracks(ov, ot, ve, te) == 1
    assert ref.set_underconstrained_views(ov, ot, ve, te) == 1 and ref.set_underconstrained_tracks(ov, ot, ve, te) == 0
    assert [int(f) for f in ve] == s.expected[3] and [int(f) for f in te] == s.expected[4]


# ------------------------------------------------------------------ the host side of the mirror
def _reconstruction(s):
    r = sfm.Reconstruction()
    r.cam_ext = np.zeros((s.num_views, 6)); r.points = np.zeros((s.num_tracks, 4))
    r.view_estimated = s.view_estimated.astype(bool); r.track_estimated = s.track_estimated.astype(bool)
    r.obs_view, r.obs_track = s.obs_view.copy(), s.obs_track.copy()
    r.obs_uv = np.zeros((len(s.obs_view), 2))
    return r


def test_single_passes_of_the_mirror_equal_the_restatement():
    s = scenes.random_sweep(60, 300, seed=3)
    r = _reconstruction(s)
    ve, te = s.view_estimated.astype(bool).tolist(), s.track_estimated.astype(bool).tolist()
    ov, ot = s.obs_view.tolist(), s.obs_track.tolist()
    for _ in range(3):
        assert inc.SetUnderconstrainedViewsToUnestimated(r) == ref.set_underconstrained_views(ov, ot, ve, te)
        assert r.view_estimated.tolist() == ve
        assert inc.SetUnderconstrainedTracksToUnestimated(r) == ref.set_underconstrained_tracks(ov, ot, ve, te)
        assert r.track_estimated.tolist() == te
    assert inc.NumEstimatedViews(r) == sum(ve) and inc.NumEstimatedTracks(r) == sum(te)


def _info(verified, homography):
    i = twoview.TwoViewInfo()
    i.num_verified_matches, i.num_homography_inliers = verified, homography
    return i


def test_order_view_pairs_ties_in_every_key():
    rows = [((0, 1), 50, 10), ((0, 2), 60, 10),      # tie in the homography inliers: more verified matches first
            ((1, 2), 60, 10),                        # tie in both: the pair decides
            ((0, 3), 40, 5),                         # fewest homography inliers: first
            ((2, 3), 30, 0),                         # not > 30: dropped
            ((1, 3), 31, 20), ((3, 4), 31, 20), ((2, 4), 31, 20)]
    expected = [(0, 3), (0, 2), (1, 2), (0, 1), (1, 3), (2, 4), (3, 4)]
    assert ref.order_view_pairs(rows, 30) == expected
    pairs = {pair: _info(v, h) for pair, v, h in reversed(rows)}
    assert inc.OrderViewPairsByInitializationCriterion(pairs, 30) == expected
    assert inc.OrderViewPairsByInitializationCriterion(list(pairs.items()), 30) == expected
    assert inc.OrderViewPairsByInitializationCriterion(pairs, 60) == []


def test_options_defaults():
    o = inc.LocalizeViewToReconstructionOptions()
    assert o.reprojection_error_threshold_pixels == 4.0 and o.assume_known_orientation is False
    assert o.bundle_adjust_view is True and o.min_num_inliers == 30 and o.pnp_type == ransac.PnPType.DLS
    d = ransac.RansacParameters()
    assert vars(o.ransac_params).keys() == vars(d).keys()
    assert all(getattr(o.ransac_params, k) == getattr(d, k) for k in vars(d))
    b = sfm.BundleAdjustmentOptions()
    assert all(getattr(o.ba_options, k) == getattr(b, k) for k in vars(b))
    assert inc.kMinNumObserved3dPoints == 30 and inc.kNumPyramidLevels == 6


def test_package_exports_the_stages():
    for name in ("FindViewsToLocalize", "VisibilityPyramid", "LocalizeViewToReconstruction", "LocalizeViewsToReconstruction",
                 "LocalizeViewToReconstructionOptions", "SetUnderconstrainedAsUnestimated", "OrderViewPairsByInitializationCriterion"):
        assert getattr(pytheiasfm_amd, name) is getattr(inc, name)
    r = sfm.Reconstruction()
    assert r.view_image_size is None and r.view_focal_prior_set is None


def test_too_few_matches_returns_before_any_device_work():
    """29 estimated tracks in the view with min_num_inliers = 30 (:141-145); no image size is needed to get there"""
    r = scenes.localization_scene()
    v = 2
    rows = np.flatnonzero(r.obs_view == v)
    r.track_estimated[r.obs_track[rows[29:]]] = False
    r.view_image_size = None
    before = r.cam_ext.copy()
    ok, summary = inc.LocalizeViewToReconstruction(v, inc.LocalizeViewToReconstructionOptions(), r)
    assert ok is False and summary.inliers == [] and summary.num_input_data_points == 0
    assert not r.view_estimated[v] and np.array_equal(r.cam_ext, before)
    assert inc.LocalizeViewsToReconstruction([v], inc.LocalizeViewToReconstructionOptions(), r)[0][0] is False


def test_missing_image_size_is_refused():
    r = scenes.localization_scene()
    r.view_image_size = None
    with pytest.raises(capi.TheiaHipError) as e:
        inc.FindViewsToLocalize(r, [2])
    assert e.value.code == INVALID
    with pytest.raises(capi.TheiaHipError) as e:
        inc.LocalizeViewToReconstruction(2, inc.LocalizeViewToReconstructionOptions(), r)
    assert e.value.code == INVALID
    with pytest.raises(capi.TheiaHipError) as e:
        inc.VisibilityPyramid(0, 480, 6)
    assert e.value.code == INVALID


def test_known_intrinsics_rule_as_written():
    r = scenes.localization_scene(num_groups=1)
    assert not inc.DoesViewHaveKnownIntrinsics(r, 2)        # unestimated: the loop re-reads THIS view (:69)
    assert inc.DoesViewHaveKnownIntrinsics(r, 1)            # estimated and shares its group
    r.view_focal_prior_set[2] = True
    assert inc.DoesViewHaveKnownIntrinsics(r, 2)
    alone = scenes.localization_scene(num_groups=6)
    assert not inc.DoesViewHaveKnownIntrinsics(alone, 1)    # estimated, but nobody shares its intrinsics


# ------------------------------------------------------------------ refusals of the two entries (no device is touched)
def _vis_args(nv=2, nt=3, levels=6):
    a = dict(off=np.array([0, 2, 3], np.int64), uv=np.array([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]]), tr=np.array([0, 2, 1], np.int32),
             est=np.ones(nt, np.uint8), size=np.array([[640, 480], [640, 480]], np.int32), n=np.full(nv, -7, np.int32),
             score=np.full(nv, -7, np.int32))
    return a


def _vis_call(a, nv=2, nt=3, levels=6, null=()):
    p = lambda k, t: capi.ptr(None if k in null else a[k], t)
    rc = capi.lib().theia_hip_visibility_scores(nv, p("off", C.c_int64), p("uv", C.c_double), p("tr", C.c_int32), nt, p("est", C.c_uint8),
                                                p("size", C.c_int32), levels, p("n", C.c_int32), p("score", C.c_int32))
    assert (a["n"] == -7).all() and (a["score"] == -7).all()        # outputs untouched
    return rc


@pytest.mark.parametrize("levels", [0, -1, 8, 100])
def test_visibility_refuses_levels_outside_1_to_7(levels):
    assert _vis_call(_vis_args(), levels=levels) == INVALID
    assert b"num_pyramid_levels" in capi.lib().theia_hip_last_error()


@pytest.mark.parametrize("size", [[0, 480], [640, 0], [-1, 480], [640, -2 ** 31]])
def test_visibility_refuses_non_positive_image_size(size):
    a = _vis_args(); a["size"][1] = size
    assert _vis_call(a) == INVALID


@pytest.mark.parametrize("track", [-1, 3, 2 ** 31 - 1])
def test_visibility_refuses_track_out_of_range(track):
    a = _vis_args(); a["tr"][2] = track
    assert _vis_call(a) == INVALID


@pytest.mark.parametrize("off", [[0, 3, 2], [-1, 2, 3], [2, 1, 3]])
def test_visibility_refuses_non_monotone_offsets(off):
    a = _vis_args(); a["off"][:] = off
    assert _vis_call(a) == INVALID


@pytest.mark.parametrize("null", ["off", "uv", "tr", "est", "size", "n", "score"])
def test_visibility_refuses_null_arrays(null):
    assert _vis_call(_vis_args(), null=(null,)) == INVALID


def test_visibility_refuses_negative_counts_and_accepts_zero_views():
    assert _vis_call(_vis_args(), nv=-1) == INVALID
    assert _vis_call(_vis_args(), nt=-1) == INVALID
    assert _vis_call(_vis_args(), nv=0, null=("off", "uv", "tr", "est", "size", "n", "score")) == 0
    assert _vis_call(_vis_args(), nv=0, levels=9) == INVALID


def _sweep_call(nv, nt, ov, ot, ve, te, null=()):
    arrs = dict(ov=np.asarray(ov, np.int32), ot=np.asarray(ot, np.int32), ve=np.asarray(ve, np.uint8), te=np.asarray(te, np.uint8))
    keep = {k: v.copy() for k, v in arrs.items()}
    p = lambda k, t: capi.ptr(None if k in null or not arrs[k].size else arrs[k], t)
    out = [C.c_int32(-7), C.c_int32(-7), C.c_int32(-7)]
    rc = capi.lib().theia_hip_set_underconstrained_unestimated(nv, nt, len(arrs["ov"]), p("ov", C.c_int32), p("ot", C.c_int32),
                                                               p("ve", C.c_uint8), p("te", C.c_uint8), C.byref(out[0]),
                                                               C.byref(out[1]), C.byref(out[2]))
    if rc:
        assert all(np.array_equal(arrs[k], keep[k]) for k in arrs) and [o.value for o in out] == [-7, -7, -7]
    return rc, [o.value for o in out]


@pytest.mark.parametrize("ov, ot", [([0, 2], [0, 1]), ([0, -1], [0, 1]), ([0, 1], [0, 2]), ([0, 1], [-1, 1])])
def test_sweep_refuses_index_out_of_range(ov, ot):
    assert _sweep_call(2, 2, ov, ot, [1, 1], [1, 1])[0] == INVALID


@pytest.mark.parametrize("null", ["ov", "ot", "ve", "te"])
def test_sweep_refuses_null_arrays(null):
    assert _sweep_call(2, 2, [0, 1], [0, 1], [1, 1], [1, 1], null=(null,))[0] == INVALID


def test_sweep_refuses_negative_counts_and_accepts_the_empty_reconstruction():
    assert _sweep_call(-1, 2, [], [], [], [1, 1])[0] == INVALID
    assert _sweep_call(2, -1, [], [], [1, 1], [])[0] == INVALID
    # no views, no tracks: the reference's loop makes one round and removes nothing; nothing is launched
    assert _sweep_call(0, 0, [], [], [], []) == (0, [0, 0, 1])
