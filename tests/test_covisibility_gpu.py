"""GPU: csrc/covisibility.hip (the view graph of a reconstruction, the MVSNet pair scores and view selection, the common
tracks of view sets) against the sequential restatement tests/covisibility_ref.py on the scenes of
tests/covisibility_scenes.py, whose preconditions tests/test_covisibility.py asserts.

Score tolerance: |device - restatement| <= num_common * 1e-12.  With theta >= 1 degree and sigma >= 1 (asserted on the
restatement), a rounding error of a few ulp in the cosine moves theta by at most about 1.3e4 ulp of a degree, the term by
at most 0.61 / sigma of that, under 1e-12; exp adds about 2 ulp of a value <= 1.  Measured differences: DESIGN.md 3.6w."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from pytheiasfm_amd import _capi as capi
from pytheiasfm_amd import covisibility as cv
from pytheiasfm_amd import sfm
from tests import alignment_ref as ar
from tests import covisibility_ref as ref
from tests import covisibility_scenes as scenes
from tests import rotation_scenes as rs

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
T0, S1, S2 = scenes.THETA0, scenes.SIGMA1, scenes.SIGMA2
INVALID = capi.THEIA_HIP_ERR_INVALID_ARGUMENT


def args(s):
    return s["num_views"], s["num_tracks"], s["obs_view"], s["obs_track"]


@functools.lru_cache(maxsize=None)
def ref_graph(name, min_shared):
    s = getattr(scenes, name)()
    return ref.view_graph(*args(s), s["view_estimated"], s["track_estimated"], min_shared, s["cam_ext"])


@functools.lru_cache(maxsize=None)
def ref_scores(name, min_shared, masked):
    s = getattr(scenes, name)()
    pairs = ref_graph(name, min_shared)[0]
    return ref.pair_scores(s["num_views"], s["obs_view"], s["obs_track"], s["cam_ext"], s["points"], pairs, T0, S1, S2,
                           s["track_estimated"] if masked else None)


def device_graph(s, min_shared, **kw):
    return cv.covisibility_graph(*args(s), s["view_estimated"], s["track_estimated"], s["cam_ext"], min_shared, **kw)


def same_bytes(a, b):
    return all(x.tobytes() == y.tobytes() and x.shape == y.shape for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------------------- graph

@pytest.mark.parametrize("name,min_shared", [("base_scene", 10), ("base_scene", 0), ("variant_scene", 10), ("variant_scene", 0)])
def test_graph_equals_the_restatement(name, min_shared):
    s = getattr(scenes, name)()
    want = ref_graph(name, min_shared)
    got = device_graph(s, min_shared)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and len(want[0]) > 0
    assert got[0].dtype == np.int32 and got[1].dtype == np.int32
    assert same_bytes(device_graph(s, min_shared), got)                                   # two calls, equal bytes
    for window in (8, 9, 1, 3, 100000):                                                   # 8 and 9: three windows at row 0
        assert same_bytes(device_graph(s, min_shared, column_window=window), got), window
    order = np.random.default_rng(99).permutation(len(s["obs_view"]))                     # the rows in another order
    shuffled = dict(s, obs_view=s["obs_view"][order], obs_track=s["obs_track"][order])
    assert same_bytes(device_graph(shuffled, min_shared), got)


def test_graph_without_flags_or_poses_and_the_capacity_convention():
    s = scenes.variant_scene()
    want = ref.view_graph(*args(s), None, None, 3)
    got = cv.covisibility_graph(*args(s), min_shared_tracks=3)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] is None and got[3] is None
    # ask with capacity 0: the count alone; a capacity one short: nothing written either
    E = len(want[0])
    count = C.c_int64(-1)
    pairs = np.full((E, 2), -7, np.int32); shared = np.full(E, -7, np.int32)
    for capacity in (0, E - 1):
        rc = capi.lib().theia_hip_covisibility_graph(
            s["num_views"], s["num_tracks"], len(s["obs_view"]), capi.ptr(s["obs_view"], C.c_int32),
            capi.ptr(s["obs_track"], C.c_int32), None, None, None, 3, 0, capacity, capi.ptr(pairs, C.c_int32),
            capi.ptr(shared, C.c_int32), None, None, C.byref(count))
        assert rc == 0 and count.value == E and (pairs == -7).all() and (shared == -7).all()


# --------------------------------------------------------------------------------------------------------- edge data

def orientation_bound():
    """tests/test_alignment_gpu.py's bound for a composition of the same rotation maps"""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rotation_maps.npz"))
    return 8.0 * float(g["err_log"]) + np.sqrt(3.0) * 8.0 * float(g["err_R"]) + 8.0 * EPS


def test_edge_data():
    s = dict(scenes.base_scene())
    cam = s["cam_ext"].copy()
    axis = np.array([0.6, -0.48, 0.64])
    cam[0, 3:6] = 5e-9 * axis                    # angle < 1e-8: ceres' small-angle branch
    cam[1, 3:6] = (np.pi - 5e-7) * axis          # within 1e-6 of pi; the pair (0, 1) has a relative rotation there too
    cam[7, :3] = cam[6, :3]                      # coincident centres
    s["cam_ext"] = cam
    pairs, shared, rot, pos = device_graph(s, 10)
    wp, ws, wrot, wpos = ref.view_graph(*args(s), None, None, 10, cam)
    assert np.array_equal(pairs, wp) and np.array_equal(shared, ws)
    assert (0, 1) in set(map(tuple, pairs.tolist()))
    coincident = (pairs[:, 0] == 6) & (pairs[:, 1] == 7)
    assert coincident.sum() == 1
    assert np.isnan(pos[coincident]).all() and np.isnan(wpos[coincident]).all() and np.isfinite(rot).all()   # passed through
    bound = orientation_bound()
    exact = np.einsum("nij,nkj->nik", ar.rotation_ld(cam[pairs[:, 1], 3:6]), ar.rotation_ld(cam[pairs[:, 0], 3:6]))
    d_exact = float(np.abs(ar.rotation_ld(rot) - exact).max())
    d_ref = float(np.abs(ar.rotation_ld(rot) - ar.rotation_ld(wrot)).max())
    d_pos = float(np.abs(pos[~coincident] - wpos[~coincident]).max())
    print(f"rotation_2 against R_j R_i' in extended precision {d_exact / EPS:.2f} eps, against the restatement "
          f"{d_ref / EPS:.2f} eps, position_2 {d_pos / EPS:.2f} eps, bound {bound / EPS:.2f} eps")
    assert d_exact <= bound and d_ref <= bound and d_pos <= bound
    assert np.linalg.norm(rot, axis=1).max() <= np.pi * (1 + 8 * EPS)
    assert np.abs(np.linalg.norm(pos[~coincident], axis=1) - 1.0).max() <= bound


# ------------------------------------------------------------------------------------------------------------ scores

@pytest.mark.parametrize("name", ["base_scene", "variant_scene"])
def test_scores_against_the_restatement(name):
    s = getattr(scenes, name)()
    pairs = ref_graph(name, 10)[0]
    want, common, smallest = ref_scores(name, 10, False)
    assert smallest >= 1.0
    score, got_common = cv.mvsnet_pair_scores(*args(s), s["cam_ext"], s["points"], pairs, T0, S1, S2)
    assert np.array_equal(got_common, common)
    ratio = np.abs(score - want) / (np.maximum(common, 1) * 1e-12)
    print(name, "largest |device - restatement|", np.abs(score - want).max(), "largest share of the bound", ratio.max())
    assert (np.abs(score - want) <= common * 1e-12).all()
    # (i, j) and (j, i) as two entries: the same bits; two runs: the same bytes
    both = np.concatenate([pairs, pairs[:, ::-1]])
    twice, _ = cv.mvsnet_pair_scores(*args(s), s["cam_ext"], s["points"], both, T0, S1, S2)
    assert twice[:len(pairs)].tobytes() == twice[len(pairs):].tobytes() == score.tobytes()
    # the mask
    wantm, commonm, _ = ref_scores(name, 10, True)
    scorem, got_commonm = cv.mvsnet_pair_scores(*args(s), s["cam_ext"], s["points"], pairs, T0, S1, S2, track_mask=s["track_estimated"])
    assert np.array_equal(got_commonm, commonm) and (np.abs(scorem - wantm) <= commonm * 1e-12).all()
    if not s["track_estimated"].all():
        assert (commonm < common).any()


def test_scores_nan_terms_and_the_sigma_branches():
    cam = np.zeros((3, 6)); cam[0, :3] = (1, 0, 0); cam[1, :3] = (-1, 0, 0); cam[2, :3] = (0.0, 1.0, 0.0)
    pts = np.array([[0.0, 2.0, 0.0, 2.0], [0.0, 40.0, 0.0, 1.0], [0.0, 3.0, 1.0, 0.0]])
    ov = np.array([0, 1, 0, 1, 2, 0], np.int32); ot = np.array([0, 0, 1, 1, 0, 2], np.int32)
    score, common = cv.mvsnet_pair_scores(3, 3, ov, ot, cam, pts, [(0, 1), (0, 2)], 5.0, 1.0, 10.0)
    want, wcommon, _ = ref.pair_scores(3, ov, ot, cam, pts, [(0, 1), (0, 2)], 5.0, 1.0, 10.0)
    # (0, 1): track 0 at 90 degrees (sigma2) and track 1 at 2.86 degrees (sigma1); (0, 2): track 0 lies on view 2's centre
    assert common.tolist() == wcommon.tolist() == [2, 1]
    assert abs(score[0] - want[0]) <= 2e-12 and want[0] > 0.09 and np.isnan(score[1]) and np.isnan(want[1])


# --------------------------------------------------------------------------------------------------------- selection

def test_selection_on_the_base_scene():
    s = scenes.base_scene()
    sel = ref.view_selection(*args(s), None, None, s["cam_ext"], s["points"], 4, T0, S1, S2)
    for row in sel.values():                                            # a condition on the scene, for every view
        assert len(row) >= 5 and all(a[0] - b[0] > 1e-6 for a, b in zip(row[:4], row[1:5]))
    neighbor, score = cv.view_selection_mvsnet(*args(s), s["view_estimated"], s["track_estimated"], s["cam_ext"], s["points"],
                                               4, T0, S1, S2)
    assert neighbor.shape == (24, 4) and score.shape == (24, 4)
    for v in range(24):
        assert neighbor[v].tolist() == [n for _, n in sel[v][:4]], v
        assert np.abs(score[v] - np.array([x for x, _ in sel[v][:4]])).max() <= 133e-12
    # the mirror's dict, and forced windows
    got = cv.ViewSelectionMVSNet(scenes.reconstruction(s), 4, T0, S1, S2)
    assert sorted(got) == list(range(24)) and all([n for _, n in got[v]] == neighbor[v].tolist() for v in got)
    again = cv.view_selection_mvsnet(*args(s), s["view_estimated"], s["track_estimated"], s["cam_ext"], s["points"], 4, T0, S1,
                                     S2, column_window=8)
    assert same_bytes(again, (neighbor, score))
    # more neighbours than any degree: -1 padding behind the whole row
    wide, wscore = cv.view_selection_mvsnet(*args(s), None, None, s["cam_ext"], s["points"], 16, T0, S1, S2)
    for v in range(24):
        want = [n for _, n in sel[v]]
        assert wide[v].tolist() == want + [-1] * (16 - len(want)) and not wscore[v, len(want):].any()


def test_selection_ties_unestimated_views_and_the_threshold():
    s = scenes.mirrored_scene()
    neighbor, score = cv.view_selection_mvsnet(*args(s), None, None, s["cam_ext"], s["points"], 3, T0, S1, S2)
    assert neighbor[0].tolist() == [1, 2, -1] and score[0, 0] == score[0, 1] > 0.0      # the tie, by view index; both stay
    assert neighbor[3].tolist() == [-1] * 3 and neighbor[4].tolist() == [-1] * 3
    assert cv.view_selection_mvsnet(*args(s), None, None, s["cam_ext"], s["points"], 3, T0, S1, S2, min_shared_tracks=16)[0].max() == -1
    v = scenes.variant_scene()
    sel = ref.view_selection(*args(v), v["view_estimated"], v["track_estimated"], v["cam_ext"], v["points"], 40, T0, S1, S2)
    neighbor, _ = cv.view_selection_mvsnet(*args(v), v["view_estimated"], v["track_estimated"], v["cam_ext"], v["points"], 3, T0,
                                           S1, S2)
    for view in range(40):
        if not v["view_estimated"][view]:
            assert neighbor[view].tolist() == [-1] * 3                                   # an unestimated view: an empty row
        else:
            row = sel[view]
            if all(a[0] - b[0] > 1e-6 for a, b in zip(row[:3], row[1:4])):
                assert neighbor[view].tolist() == ([n for _, n in row[:3]] + [-1] * 3)[:3], view
            assert not set(neighbor[view].tolist()) & set(np.flatnonzero(~v["view_estimated"]).tolist())
    got = cv.ViewSelectionMVSNet(scenes.reconstruction(v), 3, T0, S1, S2)
    assert sorted(got) == np.flatnonzero(v["view_estimated"]).tolist() and got[13] == [] and got[29] == []


# ----------------------------------------------------------------------------------------------------- common tracks

def test_common_tracks():
    s = scenes.base_scene()
    queries = scenes.common_track_queries(s)
    want = ref.find_common_tracks(24, s["obs_view"], s["obs_track"], queries)
    got = cv.find_common_tracks(*args(s), queries)
    assert [a.tolist() for a in got] == want and want[0] == [] and want[1]
    rec = scenes.reconstruction(s)
    assert cv.FindCommonTracksInViews(rec, queries[5]) == want[5]
    v = scenes.variant_scene()                                                   # unestimated tracks count, empty views too
    vq = [[13, 4], [0, 39], [3, 4, 5, 6, 7, 8], list(range(12)) + [14]]
    vwant = ref.find_common_tracks(40, v["obs_view"], v["obs_track"], vq)
    assert [a.tolist() for a in cv.find_common_tracks(*args(v), vq)] == vwant and vwant[0] == [] and 0 in vwant[3]


# -------------------------------------------------------------------------------------------------- through the stack

def test_view_graph_feeds_the_rotation_stage():
    s = scenes.base_scene()
    view_pairs = cv.ViewGraphFromReconstruction(scenes.reconstruction(s), 10)
    want = ref_graph("base_scene", 10)
    assert list(view_pairs) == list(map(tuple, want[0].tolist()))
    assert [info.num_verified_matches for info in view_pairs.values()] == want[1].tolist()
    assert sfm.RemoveDisconnectedViewPairs(view_pairs) == set() and len(view_pairs) == len(want[0])
    seed = sfm.OrientationsFromMaximumSpanningTree(view_pairs)
    assert sorted(seed) == list(range(24))
    est = sfm.NonlinearRotationEstimator()
    out = est.EstimateRotations(view_pairs, seed)
    assert est.last_success is True
    got = np.array([out[v] for v in range(24)])
    err = np.radians(rs.aligned_errors_deg(got, s["cam_ext"][:, 3:6])).max()
    print("aligned orientation error (rad, max):", err, "iterations", est.last_summary.iterations, "final cost",
          est.last_summary.final_cost)
    assert err <= 1e-8          # the orientation bound of tests/test_nonlinear_rotations_gpu.py


# ----------------------------------------------------------------------------------------------------------- refusals

def P(a, ct):
    return capi.ptr(a, ct)


def test_refusals_leave_the_outputs_untouched():
    s = scenes.base_scene()
    L = capi.lib()
    V, T, ov, ot = args(s)
    N = len(ov)
    cam, pts = np.ascontiguousarray(s["cam_ext"]), np.ascontiguousarray(s["points"])
    ve, te = s["view_estimated"].astype(np.uint8), s["track_estimated"].astype(np.uint8)
    bad_view = ov.copy(); bad_view[17] = V
    bad_track = ot.copy(); bad_track[5] = -1
    nan = float("nan")
    cap = 400
    pairs = np.full((cap, 2), -7, np.int32); shared = np.full(cap, -7, np.int32)
    rot = np.full((cap, 3), -7.0); pos = np.full((cap, 3), -7.0)
    count = C.c_int64(-7)
    i4, f8, u1 = C.c_int32, C.c_double, C.c_uint8

    def graph(V=V, T=T, N=N, ov=ov, ot=ot, cam=cam, min_shared=10, window=0, cap=cap, pairs=pairs, count=C.byref(count)):
        return L.theia_hip_covisibility_graph(V, T, N, P(ov, i4), P(ot, i4), P(ve, u1), P(te, u1), P(cam, f8), min_shared, window,
                                              cap, P(pairs, i4), P(shared, i4), P(rot, f8), P(pos, f8), count)

    for name, rc in {"negative views": graph(V=-1), "negative tracks": graph(T=-1), "negative observations": graph(N=-1),
                     "view out of range": graph(ov=bad_view), "track out of range": graph(ot=bad_track),
                     "null observations": graph(ov=None), "null pairs": graph(pairs=None), "null count": graph(count=None),
                     "negative threshold": graph(min_shared=-1), "negative window": graph(window=-1),
                     "negative capacity": graph(cap=-1), "edge data without poses": graph(cam=None)}.items():
        assert rc == INVALID, name
    assert (pairs == -7).all() and (shared == -7).all() and (rot == -7).all() and (pos == -7).all() and count.value == -7

    E = 3
    plist = np.array([[0, 1], [2, 1], [5, 4]], np.int32)
    score = np.full(E, -7.0); common = np.full(E, -7, np.int32)

    def scores(V=V, N=N, ov=ov, cam=cam, pts=pts, E=E, plist=plist, t0=T0, s1=S1, s2=S2, score=score):
        return L.theia_hip_mvsnet_pair_scores(V, T, N, P(ov, i4), P(ot, i4), P(cam, f8), P(pts, f8), None, E, P(plist, i4), t0, s1,
                                              s2, P(score, f8), P(common, i4))

    twice = plist.copy(); twice[1] = (3, 3)
    beyond = plist.copy(); beyond[2] = (0, V)
    for name, rc in {"negative pairs": scores(E=-1), "negative views": scores(V=-1), "view out of range": scores(ov=bad_view),
                     "null poses": scores(cam=None), "null points": scores(pts=None), "null pairs": scores(plist=None),
                     "null score": scores(score=None), "one view twice": scores(plist=twice), "pair out of range": scores(plist=beyond),
                     "nan theta0": scores(t0=nan), "nan sigma1": scores(s1=nan), "nan sigma2": scores(s2=nan),
                     "zero sigma1": scores(s1=0.0), "zero sigma2": scores(s2=0.0)}.items():
        assert rc == INVALID, name
    assert (score == -7).all() and (common == -7).all()

    k = 4
    neighbor = np.full((V, k), -7, np.int32); nscore = np.full((V, k), -7.0)

    def select(V=V, N=N, ot=ot, cam=cam, pts=pts, min_shared=10, k=k, t0=T0, s1=S1, s2=S2, window=0, neighbor=neighbor):
        return L.theia_hip_view_selection_mvsnet(V, T, N, P(ov, i4), P(ot, i4), P(ve, u1), P(te, u1), P(cam, f8), P(pts, f8),
                                                 min_shared, k, t0, s1, s2, window, P(neighbor, i4), P(nscore, f8))

    for name, rc in {"negative neighbours": select(k=-1), "negative views": select(V=-1), "negative observations": select(N=-1),
                     "track out of range": select(ot=bad_track), "null poses": select(cam=None), "null points": select(pts=None),
                     "null output": select(neighbor=None), "negative threshold": select(min_shared=-1),
                     "negative window": select(window=-1), "nan theta0": select(t0=nan), "nan sigma1": select(s1=nan),
                     "nan sigma2": select(s2=nan), "zero sigma1": select(s1=0.0), "zero sigma2": select(s2=0.0)}.items():
        assert rc == INVALID, name
    assert (neighbor == -7).all() and (nscore == -7).all()

    Q = 3
    offsets = np.array([0, 2, 5, 7], np.int64); qviews = np.array([0, 1, 4, 5, 6, 9, 9], np.int32)
    track_off = np.full(Q + 1, -7, np.int64); tracks = np.full(64, -7, np.int32); found = C.c_int64(-7)

    def common_tracks(V=V, N=N, ov=ov, Q=Q, offsets=offsets, qviews=qviews, cap=64, tracks=tracks, track_off=track_off):
        return L.theia_hip_find_common_tracks(V, T, N, P(ov, i4), P(ot, i4), Q, P(offsets, C.c_int64), P(qviews, i4), cap,
                                              P(track_off, C.c_int64), P(tracks, i4), C.byref(found))

    short = np.array([0, 2, 3, 7], np.int64)
    shifted = np.array([1, 3, 5, 7], np.int64)
    far = qviews.copy(); far[3] = V
    for name, rc in {"negative queries": common_tracks(Q=-1), "negative views": common_tracks(V=-1),
                     "view out of range": common_tracks(ov=bad_view), "null offsets": common_tracks(offsets=None),
                     "null views": common_tracks(qviews=None), "null tracks": common_tracks(tracks=None),
                     "null track_off": common_tracks(track_off=None), "negative capacity": common_tracks(cap=-1),
                     "a query of one view": common_tracks(offsets=short), "offsets not from 0": common_tracks(offsets=shifted),
                     "query view out of range": common_tracks(qviews=far)}.items():
        assert rc == INVALID, name
    assert (track_off == -7).all() and (tracks == -7).all() and found.value == -7
    # and the same arguments unbroken are accepted
    assert graph() == 0 and scores() == 0 and select() == 0 and common_tracks() == 0
    assert count.value == len(ref_graph("base_scene", 10)[0]) and (neighbor >= 0).all() and found.value == track_off[Q] >= 0
