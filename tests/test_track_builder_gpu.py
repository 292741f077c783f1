"""GPU: the track builder (csrc/track_builder.hip: TrackBuilder::BuildTracks, sfm/track_builder.cc:62-77, :156-209, for a whole
match graph) against the sequential restatement in tests/track_builder_ref.py.  Everything is integer: every comparison is
np.array_equal on the four output arrays and equality of every stats field; no tolerance appears."""
import ctypes as C
import functools

import numpy as np
import pytest

from pytheiasfm_amd import _capi as capi, ba, matching, sfm, synth, tracks
from tests import track_builder_cases as cases, track_builder_ref as ref

pytestmark = pytest.mark.gpu


def check(graph, min_len=2, max_len=50, want=None):
    """build_tracks on the device == the restatement, array for array and stat for stat; returns the device result"""
    got = tracks.build_tracks(*graph, tracks.TrackBuilderOptions(min_len, max_len))
    want = ref.build_tracks(*graph, min_len, max_len) if want is None else want
    for name, g, w in zip(("track_off", "obs_view", "obs_feature", "obs_track"), got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w), name
    assert got[4] == want[4]
    assert tuple(got[4]) == ref.STATS
    return got


@functools.lru_cache(maxsize=None)
def random_graph(seed):
    return cases.random_match_graph(seed)


@functools.lru_cache(maxsize=None)
def random_graph_ref(seed, max_len):
    return ref.build_tracks(*random_graph(seed), 2, max_len)


# ------------------------------------------------------------------------------------------------ 1. read-off cases
@pytest.mark.parametrize("case", cases.READ_OFF, ids=cases.READ_OFF_IDS)
def test_read_off_cases(case):
    _, _, _, min_len, max_len, expected, stats = case
    graph = cases.read_off_input(case)
    track_off, obs_view, obs_feature, _, got = check(graph, min_len, max_len)
    assert ref.tracks_as_sets(graph[0], track_off, obs_view, obs_feature) == sorted(expected)
    assert {k: got[k] for k in stats} == stats


# ------------------------------------------------------------------------------------------------ 2. random match graphs
@pytest.mark.parametrize("max_len", [6, 50])
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_random_match_graphs(seed, max_len):
    want = random_graph_ref(seed, max_len)
    stats = want[4]
    # conditions of the scene: both routes and the one-feature-per-view rule are exercised
    if max_len == 6:
        assert stats["num_oversized_components"] > 0 and stats["num_replayed_correspondences"] > 0
    else:
        assert stats["num_oversized_components"] == 0 and stats["num_replayed_correspondences"] == 0
    assert stats["num_inconsistent_features"] > 0
    print(f"seed {seed} max {max_len}: {stats}")
    check(random_graph(seed), 2, max_len, want)


# ------------------------------------------------------------------------------------------------ 3. the cap's boundary
@pytest.mark.parametrize("max_len", [2, 5, 50])
def test_cap_boundary(max_len):
    """a component of exactly max_len nodes is not oversized (no replay); one of max_len + 1 nodes is"""
    got = check(cases.cap_boundary_graph(max_len), 2, max_len)
    assert got[4]["num_components"] == 2 and got[4]["num_oversized_components"] == 1
    assert got[4]["num_replayed_correspondences"] == max_len      # the edges of the longer chain alone
    assert got[0][1] == max_len                                    # the first track is the whole shorter chain


# ------------------------------------------------------------------------------------------------ 4. shapes that stress the hooking
@pytest.mark.parametrize("max_len", [10 ** 6, 50])
def test_shuffled_path(max_len):
    """3 000 nodes in a path, its edges shuffled: trees deeper than a wave, spread over many workgroups"""
    got = check(cases.path_graph(3000, seed=5), 2, max_len)
    if max_len > 3000:
        assert got[4]["num_tracks"] == 1 and got[4]["num_observations"] == 3000 and got[4]["num_oversized_components"] == 0
    else:
        assert got[4]["num_oversized_components"] == 1 and got[4]["num_replayed_correspondences"] == 2999


def test_star():
    """5 000 edges on one hub feature: every hook contends for one root"""
    got = check(cases.star_graph(5000), 2, 10 ** 6)
    assert got[4]["num_components"] == 1 and got[4]["num_nodes"] == 5001
    assert got[4]["num_observations"] == 51 and got[4]["num_inconsistent_features"] == 4950


def test_every_edge_three_times():
    feat_off, pv1, pv2, match_off, f1, f2 = random_graph(0)
    tripled = (feat_off, pv1, pv2, 3 * match_off, np.repeat(f1, 3), np.repeat(f2, 3))
    for max_len in (6, 50):
        got = check(tripled, 2, max_len)
        once = random_graph_ref(0, max_len)
        assert all(np.array_equal(g, w) for g, w in zip(got[:4], once[:4]))     # a repeated edge changes no partition
        assert got[4]["num_replayed_correspondences"] == 3 * once[4]["num_replayed_correspondences"]


def test_many_disjoint_matches():
    """70 000 two-node components: more nodes than one launch wave of workgroups; the order of the tracks does not follow the
    order of the matches"""
    a = check(cases.disjoint_matches(70000, seed=8))
    b = tracks.build_tracks(*cases.disjoint_matches(70000, seed=8, shuffle_seed=9))
    assert a[4]["num_tracks"] == 70000 and a[4]["num_observations"] == 140000
    assert all(np.array_equal(x, y) for x, y in zip(a[:4], b[:4])) and a[4] == b[4]


# ------------------------------------------------------------------------------------------------ 5. order dependence
def test_order_dependence():
    """one edge multiset at max 6 in two pair orders: each equals its own restatement, and the two differ"""
    first = random_graph(1)
    second = cases.permute_pairs(first, seed=4)
    a = check(first, 2, 6, random_graph_ref(1, 6))
    b = check(second, 2, 6)
    assert not (len(a[1]) == len(b[1]) and all(np.array_equal(x, y) for x, y in zip(a[:4], b[:4])))


# ------------------------------------------------------------------------------------------------ 6. determinism
def test_determinism():
    graph = random_graph(2)
    for max_len in (6, 50):
        a = tracks.build_tracks(*graph, tracks.TrackBuilderOptions(2, max_len))
        b = tracks.build_tracks(*graph, tracks.TrackBuilderOptions(2, max_len))
        assert all(np.array_equal(x, y) for x, y in zip(a[:4], b[:4])) and a[4] == b[4]
    # without an effective cap the partition does not depend on the order
    free = tracks.TrackBuilderOptions(2, 10 ** 6)
    a = tracks.build_tracks(*graph, free)
    b = tracks.build_tracks(*cases.permute_pairs(graph, seed=6), free)
    assert a[4]["num_oversized_components"] == 0
    assert all(np.array_equal(x, y) for x, y in zip(a[:4], b[:4])) and a[4] == b[4]


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_leave_the_outputs_untouched():
    feat_off = np.array([0, 4, 8], np.int64)
    P = capi.ptr

    def call(pv1, pv2, match_off, f1, f2, min_len=2, max_len=50):
        pv1 = np.array(pv1, np.int32); pv2 = np.array(pv2, np.int32); match_off = np.array(match_off, np.int64)
        f1 = np.array(f1, np.int32); f2 = np.array(f2, np.int32)
        o = capi.TrackBuilderOptions(min_len, max_len)
        out = [np.full(8, -7, np.int64)] + [np.full(8, -7, np.int32) for _ in range(3)]
        st = capi.TrackBuilderStats(num_tracks=-7)
        rc = capi.lib().theia_hip_build_tracks(2, P(feat_off, C.c_int64), len(pv1), P(pv1, C.c_int32), P(pv2, C.c_int32),
                                               P(match_off, C.c_int64), P(f1, C.c_int32), P(f2, C.c_int32), C.byref(o),
                                               P(out[0], C.c_int64), P(out[1], C.c_int32), P(out[2], C.c_int32), P(out[3], C.c_int32),
                                               C.byref(st))
        return rc, out, st

    rc, out, st = call([0], [1], [0, 2], [0, 1], [0, 1])      # the call itself works
    assert rc == 0 and st.num_tracks == 2 and out[0][:3].tolist() == [0, 2, 4]
    for args, kw in ((([1], [1], [0, 1], [0], [1]), {}),                       # an edge inside one view
                     (([0], [1], [0, 2], [0, 4], [0, 1]), {}),                 # a feature index one past its view
                     (([0], [1], [0, 2], [0, 1], [-1, 1]), {}),                # a negative feature index
                     (([0], [1], [0, 2], [0, 1], [0, 1]), dict(min_len=1)),
                     (([0], [1], [0, 2], [0, 1], [0, 1]), dict(max_len=0))):
        rc, out, st = call(*args, **kw)
        assert rc == capi.THEIA_HIP_ERR_INVALID_ARGUMENT, (args, kw)
        assert all((a == -7).all() for a in out) and st.num_tracks == -7, (args, kw)
    with pytest.raises(capi.TheiaHipError):
        tracks.build_tracks(feat_off, [0], [1], [0, 1], [0], [4])
    got = tracks.build_tracks(feat_off, [], [], [0], [], [])    # zero pairs
    assert got[0].tolist() == [0] and all(len(a) == 0 for a in got[1:4]) and got[4]["num_tracks"] == 0


# ------------------------------------------------------------------------------------------------ 8. the mirror
def mirror_scene(seed=3, num_views=5, points=40):
    """per view, the image coordinates of the points it sees; correspondences between every two views over the points they share"""
    rng = np.random.default_rng(seed)
    visible = rng.random((num_views, points)) < 0.6
    xy = rng.uniform(0, 1000, (num_views, points, 2))
    return [(i, j, [p for p in range(points) if visible[i, p] and visible[j, p]])
            for i in range(num_views) for j in range(i + 1, num_views)], xy


def test_mirror_equals_build_tracks():
    corr, xy = mirror_scene()
    tb = sfm.TrackBuilder(3, 4)
    for i, j, shared in corr:
        for p in shared:
            tb.AddFeatureCorrespondence(i, tracks.Feature(xy[i, p], np.diag([1.0 + p, 2.0])), j, xy[j, p])
    recon = sfm.Reconstruction()
    recon.cam_ext = np.zeros((5, 6)); recon.view_estimated = np.ones(5, bool); recon.view_group = np.zeros(5, np.int32)
    recon.points = np.ones((2, 4)); recon.track_estimated = np.ones(2, bool); recon.track_reference_view = np.zeros(2, np.int64)
    recon.inverse_depth = np.zeros(2); recon.track_reference_bearing = np.zeros((2, 3))
    recon.obs_view = np.array([0, 1], np.int32); recon.obs_track = np.array([0, 1], np.int32)
    recon.obs_uv = np.zeros((2, 2)); recon.obs_cov = np.ones((2, 2))
    tb.BuildTracks(recon)
    # the indexed form of the same data, made here: a view numbers its points in the order in which they first appear
    index = [{} for _ in range(5)]
    first_cov = {}
    for i, j, shared in corr:
        for p in shared:
            for side, v in enumerate((i, j)):
                if p not in index[v]:
                    index[v][p] = len(index[v])
                    first_cov[v, index[v][p]] = [1.0 + p, 2.0] if side == 0 else [1.0, 1.0]
    pairs = [((i, j), [(index[i][p], index[j][p]) for p in shared]) for i, j, shared in corr]
    feat_off = np.concatenate([[0], np.cumsum([len(d) for d in index])]).astype(np.int64)
    point_of = [{f: p for p, f in d.items()} for d in index]
    track_off, obs_view, obs_feature, obs_track, stats = check((feat_off,) + ref.csr(pairs), 3, 4)
    assert stats["num_tracks"] > 0 and stats["num_oversized_components"] > 0 and tb.stats_["num_tracks"] == stats["num_tracks"]
    nt, no = stats["num_tracks"], stats["num_observations"]
    assert recon.NumTracks() == 2 + nt and len(recon.obs_view) == 2 + no
    assert np.array_equal(recon.obs_view[2:], obs_view) and np.array_equal(recon.obs_track[2:], obs_track + 2)
    assert np.array_equal(recon.obs_uv[2:], np.array([xy[v, point_of[v][f]] for v, f in zip(obs_view, obs_feature)]))
    assert not recon.track_estimated[2:].any() and recon.track_estimated[:2].all()
    assert np.array_equal(recon.track_reference_view[2:], obs_view[track_off[:-1]])
    for name in ("points", "track_estimated", "track_reference_view", "inverse_depth", "track_reference_bearing"):
        assert len(getattr(recon, name)) == 2 + nt, name
    assert len(recon.obs_uv) == len(recon.obs_cov) == len(recon.obs_track) == 2 + no
    # the covariance given with a point's first appearance in a view stays with the observation
    assert np.array_equal(recon.obs_cov[2:], np.array([first_cov[int(v), int(f)] for v, f in zip(obs_view, obs_feature)]))
    with pytest.raises(capi.TheiaHipError) as e:
        tb.BuildTracksIncremental(recon)
    assert e.value.code == capi.THEIA_HIP_ERR_UNSUPPORTED


def test_wrapper_functions():
    f1 = [np.array([10.0, 20.0]), np.array([30.0, 40.0])]; f2 = [np.array([11.0, 21.0]), np.array([31.0, 41.0])]
    f3 = [np.array([12.0, 22.0]), np.array([32.0, 42.0])]
    for add, wrap in ((sfm.AddFeatureCorrespondencesToTrackBuilder, lambda f: f),
                      (sfm.AddFullFeatureCorrespondencesToTrackBuilder, lambda f: [tracks.Feature(x, 4.0 * np.eye(2)) for x in f])):
        tb = sfm.TrackBuilder(2, 50)
        add(0, wrap(f1), 1, wrap(f2), tb)
        add(1, wrap(f2), 2, wrap(f3), tb)
        recon = sfm.Reconstruction()
        recon.cam_ext = np.zeros((3, 6))
        tb.BuildTracks(recon)
        assert recon.NumTracks() == 2 and recon.obs_view.tolist() == [0, 1, 2, 0, 1, 2] and recon.obs_track.tolist() == [0, 0, 0, 1, 1, 1]
        assert np.array_equal(recon.obs_uv, np.array([f1[0], f2[0], f3[0], f1[1], f2[1], f3[1]]))
        assert np.array_equal(recon.obs_cov, np.full((6, 2), 1.0 if add is sfm.AddFeatureCorrespondencesToTrackBuilder else 4.0))
        with pytest.raises(capi.TheiaHipError):
            add(0, wrap(f1), 1, wrap(f2)[:1], tb)


# ------------------------------------------------------------------------------------------------ 9. inside the pipeline
def descriptor_scene(seed=11, num_images=4, points=120, extra=50, dim=128, noise=0.02):
    """Unit descriptors: every point has a base descriptor and is seen by at least two images, each with its own small
    perturbation (a true pair lies at d ~ 2 dim noise^2 = 0.1, everything else at d ~ 2); every image adds `extra` unrelated
    descriptors and shuffles its features.  Returns (descriptors per image, {point: {image: feature}})."""
    rng = np.random.default_rng(seed)
    unit = lambda v: (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    base = unit(rng.standard_normal((points, dim)))
    visible = rng.random((num_images, points)) < 0.7
    for p in range(points):
        while visible[:, p].sum() < 2:
            visible[rng.integers(num_images), p] = True
    descs, truth = [], {p: {} for p in range(points)}
    for i in range(num_images):
        seen = np.nonzero(visible[i])[0]
        d = np.concatenate([unit(base[seen] + noise * rng.standard_normal((len(seen), dim))), unit(rng.standard_normal((extra, dim)))])
        perm = rng.permutation(len(d))
        descs.append(np.ascontiguousarray(d[perm]))
        where = np.argsort(perm)
        for k, p in enumerate(seen):
            truth[int(p)][i] = int(where[k])
    return descs, truth


def test_matcher_to_tracks_to_track_statistics():
    descs, truth = descriptor_scene()
    pairs = [(i, j) for i in range(4) for j in range(i + 1, 4)]
    opt = matching.FeatureMatcherOptions()
    opt.min_num_feature_matches = 1
    ok, match_off, f1, f2, _ = matching.brute_force_match_pairs(descs, pairs, opt)
    assert ok.all()
    feat_off = np.concatenate([[0], np.cumsum([len(d) for d in descs])]).astype(np.int64)
    graph = (feat_off, np.array([p[0] for p in pairs], np.int32), np.array([p[1] for p in pairs], np.int32), match_off, f1, f2)
    track_off, obs_view, obs_feature, obs_track, stats = check(graph)
    want = sorted(tuple(sorted(seen.items())) for seen in truth.values())
    assert ref.tracks_as_sets(feat_off, track_off, obs_view, obs_feature) == want
    assert stats["num_inconsistent_features"] == 0 and stats["num_small_components"] == 0
    # the tracks as a theia_ba_problem: the points of the scene seen by four cameras, every feature at its point's projection
    rng = np.random.default_rng(12)
    track_point = {tuple(sorted(seen.items())): p for p, seen in truth.items()}
    point_of_track = np.array([track_point[t] for t in (tuple((int(obs_view[i]), int(obs_feature[i])) for i in
                                                              range(track_off[k], track_off[k + 1])) for k in range(len(want)))])
    world = np.column_stack([rng.uniform(-2, 2, (len(truth), 2)), rng.uniform(5, 9, len(truth)), np.ones(len(truth))])
    cams = np.zeros((4, 6)); cams[:, 0] = [-1.0, -0.3, 0.4, 1.0]
    intr = np.array([[500.0, 1.0, 0.0, 500.0, 500.0, 0.0, 0.0]])
    points = world[point_of_track]
    uv, in_front = synth.project(0, np.repeat(intr, len(obs_view), 0), cams[obs_view], points[obs_track])
    assert in_front.all()
    fp = capi.FlatProblem(cams, intr, [0], [0, 0, 0, 0], points, uv, obs_view, obs_track)
    err, behind, min_cos = ba.track_statistics(fp)
    assert len(err) == stats["num_tracks"] and (behind == 0).all() and (err < 1e-12).all() and (min_cos < 1.0).all()
