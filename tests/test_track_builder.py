"""CPU: the track builder's rule on cases whose answer can be read off (through the sequential restatement in
tests/track_builder_ref.py), the ABI of theia_hip_build_tracks, and the host side of the pyTheia-named mirror in
pytheiasfm_amd/tracks.py.  The device code is tested in tests/test_track_builder_gpu.py."""
import ctypes as C

import numpy as np
import pytest

from tests import track_builder_cases as cases, track_builder_ref as ref


@pytest.mark.parametrize("case", cases.READ_OFF, ids=cases.READ_OFF_IDS)
def test_restatement_on_read_off_cases(case):
    _, _, _, min_len, max_len, tracks, stats = case
    graph = cases.read_off_input(case)
    track_off, obs_view, obs_feature, obs_track, got = ref.build_tracks(*graph, min_len, max_len)
    assert ref.tracks_as_sets(graph[0], track_off, obs_view, obs_feature) == sorted(tracks)
    # the stated orders: tracks by their smallest node id, observations by node id
    node = graph[0][obs_view] + obs_feature
    assert all(np.all(np.diff(node[track_off[t]:track_off[t + 1]]) > 0) for t in range(len(tracks)))
    assert np.all(np.diff(node[track_off[:-1]]) > 0)
    assert np.array_equal(obs_track, np.repeat(np.arange(len(tracks)), np.diff(track_off)))
    assert got["num_tracks"] == len(tracks) and got["num_observations"] == sum(len(t) for t in tracks)
    assert {k: got[k] for k in stats} == stats


def test_restatement_depends_on_the_edge_order():
    a, b = cases.READ_OFF[-2], cases.READ_OFF[-1]
    assert sorted(map(str, a[2])) == sorted(map(str, b[2]))     # the same edges
    ra = ref.build_tracks(*cases.read_off_input(a), a[3], a[4])
    rb = ref.build_tracks(*cases.read_off_input(b), b[3], b[4])
    assert ra[4]["num_tracks"] == 1 and rb[4]["num_tracks"] == 2


def test_restatement_refuses_what_the_rule_refuses():
    graph = cases.read_off_input(cases.READ_OFF[0])
    for min_len, max_len in ((1, 50), (2, 0), (0, -1)):
        with pytest.raises(ref.Refused):
            ref.build_tracks(*graph, min_len, max_len)
    feat_off = graph[0]
    with pytest.raises(ref.Refused):   # an edge inside one view
        ref.build_tracks(feat_off, *ref.csr([((1, 1), [(0, 1)])]))
    with pytest.raises(ref.Refused):   # a feature index outside its view
        ref.build_tracks(feat_off, *ref.csr([((0, 1), [(0, cases.FEATURES_PER_VIEW)])]))
    with pytest.raises(ref.Refused):   # a view outside [0, num_views)
        ref.build_tracks(feat_off, *ref.csr([((0, 3), [(0, 0)])]))


def test_cap_boundary_in_the_restatement():
    """a component of exactly max nodes is not oversized, one of max + 1 is"""
    stats = ref.build_tracks(*cases.cap_boundary_graph(5), 2, 5)[4]
    assert stats["num_components"] == 2 and stats["num_oversized_components"] == 1 and stats["num_replayed_correspondences"] == 5


def test_struct_sizes_and_defaults():
    from pytheiasfm_amd import _capi as capi
    assert C.sizeof(capi.TrackBuilderOptions) == 2 * 4
    assert C.sizeof(capi.TrackBuilderStats) == 8 * 8
    assert [name for name, _ in capi.TrackBuilderStats._fields_] == list(ref.STATS)
    o = capi.TrackBuilderOptions()
    capi.lib().theia_hip_track_builder_options_default(C.byref(o))
    assert (o.min_track_length, o.max_track_length) == (2, 50)    # reconstruction_builder.h:81-85
    for name in ("theia_hip_track_builder_options_default", "theia_hip_build_tracks", "theia_hip_track_builder_last_timings"):
        assert name in capi.EXPORTED_SYMBOLS and hasattr(capi.lib(), name)
    from pytheiasfm_amd import tracks
    m = tracks.TrackBuilderOptions()
    assert (m.min_track_length, m.max_track_length) == (2, 50)
    assert (m.to_c().min_track_length, m.to_c().max_track_length) == (2, 50)


def test_arguments_are_refused_before_the_device_is_touched():
    """every refusal that needs no look at the matches answers without a device, with the outputs as they were"""
    from pytheiasfm_amd import _capi as capi
    feat_off = np.array([0, 4, 8], np.int64)
    P = capi.ptr

    def call(pv1, pv2, match_off, f1, f2, min_len=2, max_len=50, feat=feat_off):
        pv1 = np.array(pv1, np.int32); pv2 = np.array(pv2, np.int32); match_off = np.array(match_off, np.int64)
        f1 = np.array(f1, np.int32); f2 = np.array(f2, np.int32)
        o = capi.TrackBuilderOptions(min_len, max_len)
        out = [np.full(8, -7, np.int64)] + [np.full(8, -7, np.int32) for _ in range(3)]
        st = capi.TrackBuilderStats(num_tracks=-7)
        rc = capi.lib().theia_hip_build_tracks(len(feat) - 1, P(feat, C.c_int64), len(pv1), P(pv1, C.c_int32), P(pv2, C.c_int32),
                                               P(match_off, C.c_int64), P(f1, C.c_int32), P(f2, C.c_int32), C.byref(o),
                                               P(out[0], C.c_int64), P(out[1], C.c_int32), P(out[2], C.c_int32), P(out[3], C.c_int32),
                                               C.byref(st))
        return rc, out, st

    bad = capi.THEIA_HIP_ERR_INVALID_ARGUMENT
    for kw in (dict(min_len=1), dict(max_len=0), dict(max_len=-3), dict(feat=np.array([0, 4, 3], np.int64)),
               dict(feat=np.array([0, 4, 2 ** 31], np.int64))):
        rc, out, st = call([0], [1], [0, 1], [0], [0], **kw)
        assert rc == bad and all((a == -7).all() for a in out) and st.num_tracks == -7, kw
    for args in (([1], [1], [0, 1], [0], [1]),           # an edge inside one view
                 ([0], [2], [0, 1], [0], [0]),           # a view outside [0, num_views)
                 ([-1], [1], [0, 1], [0], [0]),
                 ([0, 0], [1, 1], [0, 2, 1], [0, 1], [0, 1])):   # match_off decreases
        rc, out, st = call(*args)
        assert rc == bad and all((a == -7).all() for a in out) and st.num_tracks == -7, args
    # zero pairs and zero matches: 0, no tracks, track_off[0] = 0, nothing else written
    for args in (([], [], [0], [], []), ([0], [1], [0, 0], [], [])):
        rc, out, st = call(*args)
        assert rc == 0 and st.num_tracks == 0 and st.num_observations == 0 and out[0][0] == 0
        assert (out[0][1:] == -7).all() and all((a == -7).all() for a in out[1:])


def test_mirror_merges_equal_coordinates_on_the_host():
    """index_features: rows (view, x, y) with equal bit patterns are one feature, numbered per view by first appearance"""
    from pytheiasfm_amd import tracks
    views = [0, 1, 0, 2, 1, 0, 2]
    xy = [(1.5, 2.0), (1.5, 2.0), (3.0, 4.0), (0.0, 0.0), (1.5, 2.0), (1.5, 2.0), (-0.0, 0.0)]
    feat_off, feature, first = tracks.index_features(views, xy, num_views=4)
    assert feat_off.tolist() == [0, 2, 3, 5, 5]                 # view 3 exists and has no feature
    assert feature.tolist() == [0, 0, 1, 0, 0, 0, 1]            # -0.0 and 0.0 differ in their bits: two features
    assert first.tolist() == [0, 2, 1, 3, 6]
    tb = tracks.TrackBuilder(2, 50)
    tb.AddFeatureCorrespondence(0, (1.5, 2.0), 1, (7.0, 7.0))
    tb.AddFeatureCorrespondence(0, tracks.Feature((9.0, 9.0), [[2.0, 0.0], [0.0, 3.0]]), 1, ((7.0, 7.0), np.eye(2)))
    tb.AddFeatureCorrespondence(1, (7.0, 7.0), 2, (1.5, 2.0))
    feat_off, pv1, pv2, match_off, f1, f2, first = tb.indexed()
    assert feat_off.tolist() == [0, 2, 3, 4]
    assert (pv1.tolist(), pv2.tolist(), match_off.tolist()) == ([0, 1], [1, 2], [0, 2, 3])   # a run between two views is one pair
    assert (f1.tolist(), f2.tolist()) == ([0, 1, 0], [0, 0, 0])
    assert first.tolist() == [0, 2, 1, 5]
    with pytest.raises(Exception):
        tb.AddFeatureCorrespondence(3, (0.0, 0.0), 3, (1.0, 1.0))
    from pytheiasfm_amd import sfm
    assert sfm.TrackBuilder is tracks.TrackBuilder
    assert sfm.AddFeatureCorrespondencesToTrackBuilder is tracks.AddFeatureCorrespondencesToTrackBuilder
    assert sfm.AddFullFeatureCorrespondencesToTrackBuilder is tracks.AddFullFeatureCorrespondencesToTrackBuilder
