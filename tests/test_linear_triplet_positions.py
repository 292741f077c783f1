"""CPU: the linear triplet position stage without a device -- the numpy restatement against ground truth on the noise-free
scenes, the scene conditions the GPU tests rely on, every refusal of theia_hip_linear_triplet_positions that is made
before the device is touched, and the Python class's id mapping and num_threads check."""
import types

import numpy as np
import pytest

from pytheiasfm_amd import _capi as capi, global_pose, sfm
from tests import linear_triplet_scenes as ls

EPS = np.finfo(float).eps


@pytest.mark.parametrize("name", ls.NOISE_FREE)
def test_reference_recovers_ground_truth(name):
    s, r = ls.scene(name)
    scale, err = ls.fit(s, r["positions"], r["estimated"], r["index"])
    print(f"{name}: scale {scale:.3e}, relative error {err:.2e}, bound {ls.recovery_bound(r):.2e}")
    assert scale > 0.0                      # after the sign vote
    assert err <= ls.recovery_bound(r)
    w = r["eigenvalues"]
    assert abs(w[0]) <= 64 * len(w) * EPS * w[-1]   # the null vector, to rounding
    assert w[1] > 1e-7 * w[-1]                       # and only one


@pytest.mark.parametrize("name", list(ls.SCENES))
def test_scene_conditions(name):
    s, r = ls.scene(name)
    assert r["gate_margin"].min() >= 1e-9            # rounding cannot flip which tracks count
    assert np.all(np.isinf(r["ftv_margin"]) | (r["ftv_margin"] >= 1e-9))   # nor the antiparallel branch's axis
    assert np.all(s["edges"][:, 0] < s["edges"][:, 1]) and len({tuple(e) for e in s["edges"]}) == len(s["edges"])
    if s["noise"] > 0.0:
        w = r["eigenvalues"]
        assert w[0] / w[1] <= 0.1           # inverse iteration gains a factor of 10 or more per step
    tri = [tuple(int(v) for v in t) for t in r["triplets"]]
    assert tri == sorted(tri)
    if name.startswith("v4_full"):
        assert len(tri) == 4 and np.all(r["common"] == 50) and np.all(r["state"] == 0)
    if name.startswith("v12_sparse"):
        assert dict(zip(tri, (int(c) for c in r["common"]))) == ls.SPARSE_COMMON
        assert np.array_equal(r["valid"], r["common"])
        assert {t: int(st) for t, st in zip(tri, r["state"]) if st} == ls.SPARSE_STATE
        assert list(np.nonzero(~r["estimated"])[0]) == [8, 9, 10, 11]
    if name == "v10_gate":
        close = [k for k, t in enumerate(tri) if t[:2] == (0, 1)]
        assert len(close) == 8
        assert all(0 < r["valid"][k] < r["common"][k] for k in close)     # the test rejects some tracks and accepts others
        assert all(r["valid"][k] == r["common"][k] for k in range(len(tri)) if k not in close)
    if name == "v14_two_components":
        assert len(tri) == 56 + 21 and np.all(r["state"][[t[2] <= 7 for t in tri]] == 0)
        assert np.all(r["state"][[t[2] > 7 for t in tri]] == 2)
        assert list(np.nonzero(~r["estimated"])[0]) == list(range(8, 14))
    if name == "v70_hub":
        assert tri == [(0, i, i + 1) for i in range(1, 69)] and np.all(r["state"] == 0)
        assert int((s["edges"][:, 0] == 0).sum()) == 69                   # an adjacency list longer than a wavefront
    if name == "v9_collinear":
        assert np.isfinite(r["ftv_margin"]).sum() >= 1                    # the branch is taken
        assert r["estimated"].all()
    if name == "v12_flip":
        _, base = ls.scene("v12_strip")
        assert np.array_equal(r["H"], base["H"])                          # the system does not see the sign
        assert r["votes"] == -base["votes"]
        # the iteration starts from 1 / sqrt(n) and so ends on the side of the positive component sum; the voted
        # positions lie on the other side, far from the boundary: the vote of the library's run is negative
        x = r["positions"][r["index"] >= 0].ravel()
        assert x.sum() / np.linalg.norm(x) < -1.0
        assert base["positions"].sum() / np.linalg.norm(base["positions"]) > 1.0


# ---- refusals: THEIA_HIP_ERR_INVALID_ARGUMENT before the device is touched, outputs untouched, summary zero

def _tiny():
    s, _ = ls.scene("v4_full")
    return dict(orientations=s["orientations"].copy(), edges=s["edges"].copy(), relative_rotations=s["rot"].copy(),
                relative_translations=s["rel"].copy(), track_offsets=s["track_offsets"].copy(),
                obs_view=s["obs_view"].copy(), obs_feature=s["obs_feature"].copy())


def _refused(args, options=None):
    out = np.full((args["orientations"].shape[0], 3), 7.0)
    rc, p, est, summ, extra = global_pose.linear_triplet_positions(options=options, positions_out=out,
                                                                   want=global_pose.LINEAR_TRIPLET_OUTPUTS, **args)
    assert rc == capi.THEIA_HIP_ERR_INVALID_ARGUMENT, rc
    assert np.all(p == 7.0) and not est.any() and extra == {}
    assert all(v == 0 for v in summ.as_dict().values())
    return capi.lib().theia_hip_last_error().decode()


def test_refuses_view_index_out_of_range():
    a = _tiny(); a["obs_view"][5] = 4
    assert "view" in _refused(a)
    a = _tiny(); a["obs_view"][0] = -1
    _refused(a)
    a = _tiny(); a["edges"][2, 1] = 4
    assert "view pair" in _refused(a)
    a = _tiny(); a["edges"][0, 0] = -1
    _refused(a)


def test_refuses_an_edge_that_is_not_ordered():
    a = _tiny(); a["edges"][1] = a["edges"][1][::-1]
    assert "first must be < second" in _refused(a)
    a = _tiny(); a["edges"][1, 1] = a["edges"][1, 0]
    assert "first must be < second" in _refused(a)


def test_refuses_a_duplicate_edge():
    a = _tiny(); a["edges"][3] = a["edges"][0]
    assert "twice" in _refused(a)


def test_refuses_non_monotone_track_offsets():
    a = _tiny(); a["track_offsets"][3] = a["track_offsets"][2] - 1
    assert "track_offsets" in _refused(a)


def test_refuses_a_track_naming_a_view_twice():
    a = _tiny(); a["obs_view"][1] = a["obs_view"][0]
    assert "twice" in _refused(a)


@pytest.mark.parametrize("iters", [0, -3])
def test_refuses_non_positive_max_power_iterations(iters):
    o = global_pose.LinearPositionEstimatorOptions(); o.max_power_iterations = iters
    assert "max_power_iterations" in _refused(_tiny(), o)


@pytest.mark.parametrize("thr", [0.0, -1e-8, float("inf"), float("nan")])
def test_refuses_a_bad_threshold(thr):
    o = global_pose.LinearPositionEstimatorOptions(); o.eigensolver_threshold = thr
    assert "eigensolver_threshold" in _refused(_tiny(), o)


def test_refuses_fewer_than_three_edges():
    a = _tiny()
    for k in ("edges", "relative_rotations", "relative_translations"):
        a[k] = a[k][:2]
    assert "fewer than 3" in _refused(a)


def test_defaults_and_names():
    o = global_pose.LinearPositionEstimatorOptions()
    assert (o.num_threads, o.max_power_iterations, o.eigensolver_threshold) == (1, 1000, 1e-8)
    assert sfm.LinearPositionEstimator is global_pose.LinearPositionEstimator
    assert sfm.LinearPositionEstimatorOptions is global_pose.LinearPositionEstimatorOptions
    with pytest.raises(ValueError, match="unknown outputs"):
        global_pose.linear_triplet_positions(want=("base_pairs",), **_tiny())


# ---- the Python class, with the array call replaced by a recorder (no device)

def _recon(obs_view, obs_track, obs_uv, nviews, ntracks):
    r = sfm.Reconstruction()
    r.cam_ext = np.zeros((nviews, 6)); r.view_estimated = np.ones(nviews, dtype=bool)
    r.view_group = np.zeros(nviews, dtype=np.int32)
    r.group_model = np.array([0], dtype=np.int32)
    intr = np.zeros((1, capi.THEIA_MAX_INTRINSICS)); intr[0, :7] = [500.0, 1.0, 0.0, 320.0, 240.0, 0.0, 0.0]
    r.group_intrinsics = intr
    r.points = np.zeros((ntracks, 4)); r.track_estimated = np.ones(ntracks, dtype=bool)
    r.obs_view = np.asarray(obs_view, dtype=np.int32); r.obs_track = np.asarray(obs_track, dtype=np.int32)
    r.obs_uv = np.asarray(obs_uv, dtype=np.float64)
    return r


def _info(k):
    return types.SimpleNamespace(rotation_2=np.array([0.1 * k, 0.0, 0.0]), position_2=np.array([1.0 * k, 2.0, 3.0]))


def test_class_maps_ids_and_unprojects(monkeypatch):
    # views 0, 2, 5 have orientations (view ids need not be dense in the dict); observations interleave the tracks
    obs_view = [5, 0, 2, 0, 5, 2]
    obs_track = [1, 0, 1, 1, 0, 0]
    uv = np.array([[320.0 + 50 * k, 240.0 - 25 * k] for k in range(6)])
    r = _recon(obs_view, obs_track, uv, nviews=6, ntracks=2)
    seen = {}

    def fake(aa, edges, rot, rel, off, ov, of, options):
        seen.update(aa=aa, edges=edges, rot=rot, rel=rel, off=off, ov=ov, of=of)
        pos = np.arange(9.0).reshape(3, 3)
        return 0, pos, np.array([True, True, False]), capi.LinearTripletSummary(), {}

    monkeypatch.setattr(global_pose, "linear_triplet_positions", fake)
    orientations = {5: np.array([0.5, 0, 0]), 0: np.array([0.0, 0, 0]), 2: np.array([0.2, 0, 0])}
    pairs = {(0, 5): _info(1), (2, 5): _info(2), (0, 2): _info(3)}
    est = global_pose.LinearPositionEstimator(global_pose.LinearPositionEstimatorOptions(), r)
    got = est.EstimatePositions(pairs, orientations)
    assert np.array_equal(seen["aa"][:, 0], [0.0, 0.2, 0.5])            # views sorted by id: 0, 2, 5 -> 0, 1, 2
    assert list(seen["off"]) == [0, 3, 6]
    assert list(seen["ov"]) == [0, 2, 1, 2, 1, 0]                       # track 0: views 0, 5, 2; track 1: 5, 2, 0
    assert np.allclose(seen["of"], (uv[[1, 4, 5, 0, 2, 3]] - [320.0, 240.0]) / 500.0, rtol=0, atol=1e-15)
    assert seen["edges"].tolist() == [[0, 2], [1, 2], [0, 1]]
    assert seen["rot"][:, 0].tolist() == [0.1, 0.2, 0.30000000000000004] and seen["rel"][:, 0].tolist() == [1.0, 2.0, 3.0]
    assert sorted(got) == [0, 2] and np.array_equal(got[2], [3.0, 4.0, 5.0])   # the view outside the system is absent
    assert isinstance(est.last_summary, capi.LinearTripletSummary)


def test_class_checks_num_threads():
    r = _recon([0, 1, 2], [0, 0, 0], np.zeros((3, 2)), nviews=3, ntracks=1)
    o = global_pose.LinearPositionEstimatorOptions(); o.num_threads = 0
    with pytest.raises(capi.TheiaHipError, match="num_threads") as ex:
        global_pose.LinearPositionEstimator(o, r)
    assert ex.value.code == capi.THEIA_HIP_ERR_INVALID_ARGUMENT


def test_class_raises_for_views_without_orientation():
    r = _recon([0, 1, 2], [0, 0, 0], np.zeros((3, 2)), nviews=3, ntracks=1)
    est = global_pose.LinearPositionEstimator(global_pose.LinearPositionEstimatorOptions(), r)
    with pytest.raises(capi.TheiaHipError, match="view 2 has no orientation") as ex:
        est.EstimatePositions({}, {0: np.zeros(3), 1: np.zeros(3)})
    assert ex.value.code == capi.THEIA_HIP_ERR_INVALID_ARGUMENT
    r = _recon([0, 1], [0, 0], np.zeros((2, 2)), nviews=3, ntracks=1)
    est = global_pose.LinearPositionEstimator(global_pose.LinearPositionEstimatorOptions(), r)
    with pytest.raises(capi.TheiaHipError, match=r"view pair \(1, 2\) names view 2") as ex:
        est.EstimatePositions({(0, 1): _info(1), (1, 2): _info(2)}, {0: np.zeros(3), 1: np.zeros(3)})
    assert ex.value.code == capi.THEIA_HIP_ERR_INVALID_ARGUMENT
    with pytest.raises(capi.TheiaHipError, match="not keyed id1 < id2"):
        est.EstimatePositions({(1, 0): _info(1)}, {0: np.zeros(3), 1: np.zeros(3)})
