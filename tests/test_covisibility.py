"""CPU: the restatement of the co-visibility rules (tests/covisibility_ref.py) against answers made by hand, the
preconditions of the scenes the GPU tests run on (tests/covisibility_scenes.py), and what pytheiasfm_amd/covisibility.py
refuses or answers without a device."""
import math

import numpy as np
import pytest

from pytheiasfm_amd import _capi as capi
from pytheiasfm_amd import covisibility as cv
from tests import covisibility_ref as ref
from tests import covisibility_scenes as scenes

# three views, twelve tracks: |0 & 1| = |{4,5,6,7}| = 4, |0 & 2| = |{0,1,6,7}| = 4, |1 & 2| = |{6,7,8,9,10}| = 5
HAND = {0: [0, 1, 2, 3, 4, 5, 6, 7], 1: [4, 5, 6, 7, 8, 9, 10, 11], 2: [0, 1, 6, 7, 8, 9, 10]}


def hand_observations():
    rows = [(v, t) for v, ts in HAND.items() for t in ts]
    rows = [rows[k] for k in np.random.default_rng(0).permutation(len(rows))]
    return np.array([r[0] for r in rows], np.int32), np.array([r[1] for r in rows], np.int32)


def hand_graph(min_shared, view_est=None, track_est=None):
    ov, ot = hand_observations()
    pairs, shared, _, _ = ref.view_graph(3, 12, ov, ot, view_est, track_est, min_shared)
    return dict(zip(map(tuple, pairs.tolist()), shared.tolist()))


def test_hand_counts_and_the_strict_threshold():
    assert hand_graph(0) == {(0, 1): 4, (0, 2): 4, (1, 2): 5}
    assert hand_graph(3) == {(0, 1): 4, (0, 2): 4, (1, 2): 5}
    assert hand_graph(4) == {(1, 2): 5}            # shared == min_shared_tracks gives no edge
    assert hand_graph(5) == {}
    track_est = np.ones(12, bool); track_est[6] = False
    assert hand_graph(0, track_est=track_est) == {(0, 1): 3, (0, 2): 3, (1, 2): 4}
    assert hand_graph(0, view_est=np.array([True, True, False])) == {(0, 1): 4}     # both views must be estimated
    assert hand_graph(0, view_est=np.array([False, True, True])) == {(1, 2): 5}


def test_right_angle_score():
    cam = np.zeros((2, 6)); cam[0, 0] = 1.0; cam[1, 0] = -1.0
    pts = np.array([[0.0, 2.0, 0.0, 2.0]])   # (0, 1, 0) after hnormalized
    assert abs(ref.angle_between_rays(cam[0, :3].tolist(), cam[1, :3].tolist(), pts[0].tolist()) - 90.0) <= 90.0 * 2 ** -52
    score, common, smallest = ref.pair_scores(2, [0, 1], [0, 0], cam, pts, [(0, 1), (1, 0)], 5.0, 1.0, 10.0)
    want = math.exp(-85.0 ** 2 / 200.0)
    assert abs(score[0] - want) <= 1e-13 * want and score[0] == score[1] and common.tolist() == [1, 1]
    assert abs(smallest - 90.0) <= 90.0 * 2 ** -52


def test_sigma_branch_on_both_sides():
    assert ref.score_fun(3.0, 5.0, 1.0, 10.0) == math.exp(-2.0)           # theta <= theta0: sigma1
    assert ref.score_fun(7.0, 5.0, 1.0, 10.0) == math.exp(-4.0 / 200.0)   # theta > theta0: sigma2
    assert ref.score_fun(5.0, 5.0, 1.0, 10.0) == 1.0
    assert ref.score_fun(5.0 + 2 ** -40, 5.0, 1e-15, 10.0) > 0.999        # just above: sigma2, or the term would vanish
    assert math.isnan(ref.score_fun(math.nan, 5.0, 1.0, 10.0))


def test_order_of_ties_and_nans():
    items = [(0.5, 3), (math.nan, 1), (0.7, 9), (0.5, 2), (math.nan, 0), (-1.0, 4)]
    got = sorted(items, key=lambda it: ref.order_key(*it))
    assert [v for _, v in got] == [9, 2, 3, 4, 0, 1]


def test_cosine_beyond_one_and_coincident_points_give_nan():
    assert math.isnan(ref.angle_between_rays([1.0, 0.0, 0.0], [2.0, 0.0, 0.0], [1.0, 0.0, 0.0, 1.0]))   # p == c_i: 0 / 0
    w, p = ref.two_view_info([1.0, 2.0, 3.0, 0.1, 0.2, 0.3], [1.0, 2.0, 3.0, 0.3, 0.2, 0.1])
    assert all(math.isnan(x) for x in p) and not any(math.isnan(x) for x in w)


def test_common_tracks_by_hand():
    ov, ot = hand_observations()
    assert ref.find_common_tracks(3, ov, ot, [[0, 1], [2, 1], [0, 1, 2], [1, 1]]) == [[4, 5, 6, 7], [6, 7, 8, 9, 10], [6, 7],
                                                                                   HAND[1]]
    with pytest.raises(AssertionError):
        ref.find_common_tracks(3, ov, ot, [[0]])


# ------------------------------------------------------------------------------------------------ the Python layer

def refused(call):
    with pytest.raises(capi.TheiaHipError) as info:
        call()
    assert info.value.code == capi.THEIA_HIP_ERR_INVALID_ARGUMENT


def test_python_layer_refusals():
    ov, ot = hand_observations()
    cam = np.zeros((3, 6)); cam[:, 0] = np.arange(3)
    pts = np.ones((12, 4))
    refused(lambda: cv.covisibility_graph(3, 12, ov, ot[:-1]))
    refused(lambda: cv.covisibility_graph(2, 12, ov, ot))                       # view 2 out of range
    refused(lambda: cv.covisibility_graph(3, 11, ov, ot))                       # track 11 out of range
    refused(lambda: cv.covisibility_graph(-1, 12, ov[:0], ot[:0]))
    refused(lambda: cv.covisibility_graph(3, 12, ov, ot, min_shared_tracks=-1))
    refused(lambda: cv.covisibility_graph(3, 12, ov, ot, column_window=-1))
    refused(lambda: cv.covisibility_graph(3, 12, ov, ot, view_estimated=np.ones(4, bool)))
    refused(lambda: cv.covisibility_graph(3, 12, ov, ot, cam_ext=np.zeros((2, 6))))
    refused(lambda: cv.mvsnet_pair_scores(3, 12, ov, ot, cam, pts, [(1, 1)], 5.0, 1.0, 10.0))
    refused(lambda: cv.mvsnet_pair_scores(3, 12, ov, ot, cam, pts, [(0, 3)], 5.0, 1.0, 10.0))
    refused(lambda: cv.mvsnet_pair_scores(3, 12, ov, ot, cam, pts, [(0, 1)], math.nan, 1.0, 10.0))
    refused(lambda: cv.mvsnet_pair_scores(3, 12, ov, ot, cam, pts, [(0, 1)], 5.0, 0.0, 10.0))
    refused(lambda: cv.mvsnet_pair_scores(3, 12, ov, ot, cam, pts, [(0, 1)], 5.0, 1.0, math.nan))
    refused(lambda: cv.view_selection_mvsnet(3, 12, ov, ot, None, None, cam, pts, -1, 5.0, 1.0, 10.0))
    refused(lambda: cv.view_selection_mvsnet(3, 12, ov, ot, None, None, cam, pts, 2, 5.0, 1.0, 0.0))
    refused(lambda: cv.find_common_tracks(3, 12, ov, ot, [[0, 1], [2]]))        # the reference's CHECK_GT
    refused(lambda: cv.find_common_tracks(3, 12, ov, ot, [[0, 3]]))


def test_empty_inputs_answer_without_a_device():
    none = np.zeros(0, np.int32)
    pairs, shared, rot, pos = cv.covisibility_graph(0, 0, none, none)
    assert pairs.shape == (0, 2) and shared.shape == (0,) and rot is None and pos is None
    pairs, shared, rot, pos = cv.covisibility_graph(3, 12, none, none, cam_ext=np.zeros((3, 6)))
    assert pairs.shape == (0, 2) and rot.shape == (0, 3) and pos.shape == (0, 3)
    ov, ot = hand_observations()
    score, common = cv.mvsnet_pair_scores(3, 12, ov, ot, np.zeros((3, 6)), np.ones((12, 4)), np.zeros((0, 2)), 5.0, 1.0, 10.0)
    assert score.shape == (0,) and common.shape == (0,)
    score, common = cv.mvsnet_pair_scores(3, 12, none, none, np.zeros((3, 6)), np.ones((12, 4)), [(0, 1), (2, 1)], 5.0, 1.0, 10.0)
    assert score.tolist() == [0.0, 0.0] and common.tolist() == [0, 0]
    neighbor, score = cv.view_selection_mvsnet(3, 12, none, none, None, None, np.zeros((3, 6)), np.ones((12, 4)), 2, 5.0, 1.0, 10.0)
    assert (neighbor == -1).all() and neighbor.shape == (3, 2) and not score.any()
    assert cv.view_selection_mvsnet(0, 0, none, none, None, None, np.zeros((0, 6)), np.zeros((0, 4)), 2, 5.0, 1.0, 10.0)[0].shape == (0, 2)
    assert [a.tolist() for a in cv.find_common_tracks(3, 12, none, none, [[0, 1], [1, 2, 0]])] == [[], []]
    assert cv.find_common_tracks(3, 12, ov, ot, []) == []


def test_mvs_module_mirrors_pt_mvs():
    from pytheiasfm_amd import mvs, sfm
    assert mvs.ViewSelectionMVSNet is cv.ViewSelectionMVSNet
    assert sfm.ViewGraphFromReconstruction is cv.ViewGraphFromReconstruction
    assert sfm.FindCommonTracksInViews is cv.FindCommonTracksInViews


# ------------------------------------------------------------------------------------- the scenes' own preconditions

def test_base_scene_preconditions():
    s = scenes.base_scene()
    assert s["num_views"] == 24 and s["num_tracks"] == 600
    per_track = np.bincount(s["obs_track"], minlength=600)
    assert per_track.min() >= 3 and per_track.max() <= 8
    assert len(set(zip(s["obs_view"].tolist(), s["obs_track"].tolist()))) == len(s["obs_view"])   # one row per (view, track)
    pairs, shared, _, _ = ref.view_graph(24, 600, s["obs_view"], s["obs_track"], None, None, 10)
    degree = np.bincount(pairs.reshape(-1), minlength=24)
    print("neighbours per view", degree.min(), degree.max(), "shared tracks per edge", shared.min(), shared.max())
    assert degree.min() >= 5 and shared.min() == 11
    # 23 columns behind row 0: three windows of 8 (8, 8, 7) and of 9 (9, 9, 5), the last one ragged
    assert [math.ceil(23 / w) for w in (8, 9)] == [3, 3] and 23 % 8 and 23 % 9
    _, common, smallest = ref.pair_scores(24, s["obs_view"], s["obs_track"], s["cam_ext"], s["points"], pairs, scenes.THETA0,
                                          scenes.SIGMA1, scenes.SIGMA2)
    print("smallest triangulation angle (degrees)", smallest)
    assert smallest >= 1.0 and min(scenes.SIGMA1, scenes.SIGMA2) >= 1.0   # the conditions of the score tolerance
    assert (common >= shared).all()
    sel = ref.view_selection(24, 600, s["obs_view"], s["obs_track"], None, None, s["cam_ext"], s["points"], 4, scenes.THETA0,
                             scenes.SIGMA1, scenes.SIGMA2)
    gap = min(a[0] - b[0] for row in sel.values() for a, b in zip(row[:4], row[1:5]))
    print("smallest gap among each view's five best scores", gap)
    assert gap > 1e-6


def test_variant_scene_preconditions():
    s = scenes.variant_scene()
    per_view = np.bincount(s["obs_view"], minlength=40)
    assert per_view[13] == 0 and per_view[29] == 0 and (np.delete(per_view, [13, 29]) > 0).all()
    assert np.bincount(s["obs_track"], minlength=900)[0] == 38                   # the hub
    assert not s["view_estimated"].all() and not s["track_estimated"].all() and s["track_estimated"][0]
    assert len(set(zip(s["obs_view"].tolist(), s["obs_track"].tolist()))) == len(s["obs_view"])
    pairs, shared, _, _ = ref.view_graph(40, 900, s["obs_view"], s["obs_track"], s["view_estimated"], s["track_estimated"], 0)
    est = np.flatnonzero(s["view_estimated"] & (per_view > 0))
    assert len(pairs) == len(est) * (len(est) - 1) // 2                          # the hub joins every estimated pair
    assert shared.min() == 1 and shared.max() > 10


def test_mirrored_scene_has_an_exact_tie():
    s = scenes.mirrored_scene()
    score, common, _ = ref.pair_scores(5, s["obs_view"], s["obs_track"], s["cam_ext"], s["points"], [(0, 1), (0, 2), (1, 2)],
                                       scenes.THETA0, scenes.SIGMA1, scenes.SIGMA2)
    assert score[0] == score[1] and score[0] > 0.0 and score[2] != score[0] and common.tolist() == [16, 16, 16]


def test_common_track_queries_cover_the_edge_cases():
    s = scenes.base_scene()
    queries = scenes.common_track_queries(s)
    assert len(queries) == 50 and all(2 <= len(q) <= 6 for q in queries)
    answers = ref.find_common_tracks(24, s["obs_view"], s["obs_track"], queries)
    assert answers[0] == [] and len(set(queries[1])) < len(queries[1]) and answers[1]
    assert sum(1 for a in answers if a) >= 25
