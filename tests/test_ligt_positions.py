"""CPU: the LiGT position stage without a device -- the numpy restatement against ground truth on the noise-free scenes,
the scene conditions the GPU tests rely on, every refusal of theia_hip_ligt_positions (all of them return before the
device is touched), and the Python class's id mapping and un-projection rule."""
import types

import numpy as np
import pytest

from pytheiasfm_amd import _capi as capi, global_pose, sfm
from tests import ligt_scenes as ls


def _fit(scene, positions, estimated, index):
    """positions = s (c - c_held): the least-squares s and the largest view error relative to |s (c - c_held)|_2."""
    held = int(np.nonzero(index == -1)[0][0])
    d = (scene["positions"] - scene["positions"][held])[estimated]
    p = positions[estimated]
    s = float((p * d).sum() / (d * d).sum())
    return s, float(np.linalg.norm(p - s * d, axis=1).max() / np.linalg.norm(s * d))


@pytest.mark.parametrize("name", ls.NOISE_FREE)
def test_reference_recovers_ground_truth(name):
    s, r = ls.scene(name)
    scale, err = _fit(s, r["positions"], r["estimated"], r["index"])
    print(f"{name}: scale {scale:.3e}, relative error {err:.2e}, bound {ls.recovery_bound(r):.2e}")
    assert scale > 0.0                      # after the sign vote
    assert err <= ls.recovery_bound(r)
    assert r["estimated"].all() and r["num_views_in_system"] == s["num_views"]
    w = r["eigenvalues"]
    assert abs(w[0]) <= 64 * len(w) * np.finfo(float).eps * w[-1]   # the null vector, to rounding
    assert w[1] > 1e-7 * w[-1]                                       # and only one


@pytest.mark.parametrize("name", list(ls.SCENES))
def test_scene_conditions(name):
    s, r = ls.scene(name)
    used = r["base_pairs"][:, 0] >= 0
    assert used.any()
    gap = r["theta_gap"][used]
    assert np.all(gap > 1e-9), gap.min()    # the base pairs are decided far above rounding
    lengths = np.diff(s["track_offsets"])
    assert np.array_equal(used, lengths >= 3)
    if name == "v20_extra":
        assert list(lengths[-3:]) == [2, 3, 20] and not used[-3] and used[-2] and used[-1]
    if name == "v70_long":
        assert lengths[-1] == 70
    if name == "v20_unused":
        assert list(np.nonzero(~r["estimated"])[0]) == [20, 21]
    if s["noise"] > 0.0:
        w = r["eigenvalues"]
        assert w[0] / w[1] <= 0.1           # inverse iteration gains a factor of 10 or more per step


# ---- refusals: THEIA_HIP_ERR_INVALID_ARGUMENT before the device is touched, outputs untouched

def _tiny():
    s, _ = ls.scene("v6")
    return dict(orientations=s["orientations"].copy(), track_offsets=s["track_offsets"].copy(),
                obs_view=s["obs_view"].copy(), obs_feature=s["obs_feature"].copy(), edges=s["edges"].copy(),
                relative_translations=s["rel"].copy())


def _refused(args, options=None):
    out = np.full((args["orientations"].shape[0], 3), 7.0)
    rc, p, est, summ, extra = global_pose.ligt_positions(options=options, positions_out=out, want=("base_pairs",), **args)
    assert rc == capi.THEIA_HIP_ERR_INVALID_ARGUMENT, rc
    assert np.all(p == 7.0) and not est.any() and extra == {}
    assert summ.num_views_in_system == 0 and summ.iterations == 0
    return capi.lib().theia_hip_last_error().decode()


def test_refuses_view_index_out_of_range():
    a = _tiny(); a["obs_view"][5] = 6
    assert "view" in _refused(a)
    a = _tiny(); a["obs_view"][0] = -1
    _refused(a)


def test_refuses_non_monotone_track_offsets():
    a = _tiny(); a["track_offsets"][3] = a["track_offsets"][2] - 1
    assert "track_offsets" in _refused(a)


def test_refuses_a_track_naming_a_view_twice():
    a = _tiny(); a["obs_view"][1] = a["obs_view"][0]
    assert "twice" in _refused(a)


def test_refuses_an_edge_out_of_range():
    a = _tiny(); a["edges"][2, 1] = 6
    assert "view pair" in _refused(a)
    a = _tiny(); a["edges"][0, 0] = -1
    _refused(a)


@pytest.mark.parametrize("iters", [0, -3])
def test_refuses_non_positive_max_power_iterations(iters):
    o = global_pose.LiGTPositionEstimatorOptions(); o.max_power_iterations = iters
    assert "max_power_iterations" in _refused(_tiny(), o)


@pytest.mark.parametrize("thr", [0.0, -1e-8, float("inf"), float("nan")])
def test_refuses_a_bad_threshold(thr):
    o = global_pose.LiGTPositionEstimatorOptions(); o.eigensolver_threshold = thr
    assert "eigensolver_threshold" in _refused(_tiny(), o)


def test_refuses_when_no_track_is_used():
    a = _tiny()
    a["track_offsets"] = np.arange(0, len(a["obs_view"]) + 1, 2, dtype=np.int32)[:11]   # ten tracks of 2 observations
    a["obs_view"] = np.tile(np.array([0, 1], dtype=np.int32), 10)
    a["obs_feature"] = a["obs_feature"][:20]
    assert "no track used" in _refused(a)


def test_defaults_and_enum():
    o = global_pose.LiGTPositionEstimatorOptions()   # LiGT_position_estimator.h:70-82
    assert (o.num_threads, o.max_power_iterations, o.eigensolver_threshold, o.max_num_views_svd) == (1, 1000, 1e-8, 500)
    assert sfm.GlobalPositionEstimatorType.LIGT == 3
    assert sfm.LiGTPositionEstimator is global_pose.LiGTPositionEstimator
    assert sfm.LiGTPositionEstimatorOptions is global_pose.LiGTPositionEstimatorOptions


# ---- the Python class, with the array call replaced by a recorder (no device)

def _recon(obs_view, obs_track, obs_uv, nviews, ntracks, model=0):
    r = sfm.Reconstruction()
    r.cam_ext = np.zeros((nviews, 6)); r.view_estimated = np.ones(nviews, dtype=bool)
    r.view_group = np.zeros(nviews, dtype=np.int32)
    r.group_model = np.array([model], dtype=np.int32)
    intr = np.zeros((1, capi.THEIA_MAX_INTRINSICS)); intr[0, :7] = [500.0, 1.0, 0.0, 320.0, 240.0, 0.0, 0.0]
    r.group_intrinsics = intr
    r.points = np.zeros((ntracks, 4)); r.track_estimated = np.ones(ntracks, dtype=bool)
    r.obs_view = np.asarray(obs_view, dtype=np.int32); r.obs_track = np.asarray(obs_track, dtype=np.int32)
    r.obs_uv = np.asarray(obs_uv, dtype=np.float64)
    return r


def test_class_maps_ids_and_unprojects(monkeypatch):
    # views 0, 2, 5 have orientations (view ids need not be dense in the dict); observations interleave the tracks
    obs_view = [5, 0, 2, 0, 5, 2]
    obs_track = [1, 0, 1, 1, 0, 0]
    uv = np.array([[320.0 + 50 * k, 240.0 - 25 * k] for k in range(6)])
    r = _recon(obs_view, obs_track, uv, nviews=6, ntracks=2)
    seen = {}

    def fake(aa, off, ov, of, edges, rel, options):
        seen.update(aa=aa, off=off, ov=ov, of=of, edges=edges, rel=rel)
        pos = np.arange(9.0).reshape(3, 3)
        return 0, pos, np.array([True, True, False]), capi.LigtSummary(), {}

    monkeypatch.setattr(global_pose, "ligt_positions", fake)
    orientations = {5: np.array([0.5, 0, 0]), 0: np.array([0.0, 0, 0]), 2: np.array([0.2, 0, 0])}
    info = types.SimpleNamespace(position_2=np.array([1.0, 2.0, 3.0]))
    pairs = {(0, 5): info, (2, 9): info}    # view 9 has no orientation: the pair does not vote
    est = global_pose.LiGTPositionEstimator(global_pose.LiGTPositionEstimatorOptions(), r)
    got = est.EstimatePositions(pairs, orientations)
    assert np.array_equal(seen["aa"][:, 0], [0.0, 0.2, 0.5])            # views sorted by id: 0, 2, 5 -> 0, 1, 2
    assert list(seen["off"]) == [0, 3, 6]
    assert list(seen["ov"]) == [0, 2, 1, 2, 1, 0]                       # track 0: views 0, 5, 2; track 1: 5, 2, 0
    assert np.allclose(seen["of"], (uv[[1, 4, 5, 0, 2, 3]] - [320.0, 240.0]) / 500.0, rtol=0, atol=1e-15)
    assert seen["edges"].tolist() == [[0, 2]] and seen["rel"].tolist() == [[1.0, 2.0, 3.0]]
    assert sorted(got) == [0, 2] and np.array_equal(got[2], [3.0, 4.0, 5.0])   # the view outside the system is absent


def test_class_takes_normalized_features_and_refuses_other_models(monkeypatch):
    r = _recon([0, 1, 2], [0, 0, 0], np.zeros((3, 2)), nviews=3, ntracks=1, model=2)
    orientations = {v: np.zeros(3) for v in range(3)}
    est = global_pose.LiGTPositionEstimator(global_pose.LiGTPositionEstimatorOptions(), r)
    with pytest.raises(capi.TheiaHipError, match="pass normalized_features") as ex:
        est.EstimatePositions({}, orientations)
    assert ex.value.code == capi.THEIA_HIP_ERR_UNSUPPORTED
    feats = np.array([[0.1, 0.2], [0.3, 0.4], [0.5, 0.6]])
    seen = {}
    monkeypatch.setattr(global_pose, "ligt_positions", lambda aa, off, ov, of, e, t, o: (
        seen.update(of=of) or (0, np.zeros((3, 3)), np.ones(3, dtype=bool), capi.LigtSummary(), {})))
    global_pose.LiGTPositionEstimator(global_pose.LiGTPositionEstimatorOptions(), r, feats).EstimatePositions({}, orientations)
    assert np.array_equal(seen["of"], feats)


def test_class_raises_for_an_observation_without_orientation():
    r = _recon([0, 1, 2], [0, 0, 0], np.zeros((3, 2)), nviews=3, ntracks=1)
    est = global_pose.LiGTPositionEstimator(global_pose.LiGTPositionEstimatorOptions(), r)
    with pytest.raises(capi.TheiaHipError, match="view 2 has no orientation"):
        est.EstimatePositions({}, {0: np.zeros(3), 1: np.zeros(3)})
