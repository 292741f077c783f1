"""CPU: the restatement of the two view-graph prunings (tests/view_graph_pruning_ref.py) on the reference's own scenes and
on edge scenes whose answers are written out here by hand; theia_hip_remove_disconnected_view_pairs, which is host code and
runs here in full, against the restatement array for array; the pyTheia-named mirror of it on the dict.  The cycle filter
itself runs on the device: tests/test_view_graph_pruning_gpu.py."""
import ctypes as C

import numpy as np
import pytest

from pytheiasfm_amd import _capi as capi
from pytheiasfm_amd import global_pose, sfm, twoview
from tests import view_graph_pruning_ref as ref

INVALID = capi.THEIA_HIP_ERR_INVALID_ARGUMENT
INF = float("inf")


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("num_invalid,pairs,tris", [(0, 30, None), (5, 35, None), (15, 45, 120)])
def test_restatement_leaves_exactly_the_valid_pairs(num_invalid, pairs, tris):
    """filter_view_graph_cycles_by_rotation_test.cc:148-161: NumEdges() == num_valid_view_pairs after the filter."""
    s = ref.reference_scene(num_invalid)
    r = s["ref"][4.0]
    assert len(s["pairs"]) == pairs and int(s["bad"].sum()) == num_invalid
    assert np.array_equal(r["removed"], s["bad"])
    assert int((~r["removed"]).sum()) == 30
    if tris is not None:
        assert r["num_triangles"] == tris   # 45 pairs on 10 views: the complete graph
    m = r["min_loop_error_degrees"]
    assert m[~s["bad"]].max() < 1e-12       # consistent loops close to rounding


def test_restatement_on_the_hub_and_dense_scenes():
    h = ref.hub_scene()
    r = h["ref"][4.0]
    assert len(h["pairs"]) == 400 and r["num_triangles"] == 200
    assert np.array_equal(r["triangles_per_pair"][:200], np.full(200, 2)) and np.array_equal(r["triangles_per_pair"][200:], np.ones(200))
    assert 0 < int(r["removed"].sum()) < 400 and int((h["pairs"][:, 0] > h["pairs"][:, 1]).sum()) == 133
    d = ref.dense_scene()
    assert len(d["pairs"]) == 3000 and int((d["pairs"][:, 0] > d["pairs"][:, 1]).sum()) == 600
    assert int(d["ref"][4.0]["triangles_per_pair"].sum()) == 3 * d["ref"][4.0]["num_triangles"]
    assert np.array_equal(d["ref"][4.0]["removed"], d["bad"])
    bulk = d["ref"][ref.DENSE_BULK_THRESHOLD]["removed"][~d["bad"]]
    assert bulk.sum() > 500 and (~bulk).sum() > 500   # both outcomes among the good pairs


# name: (removed at 4 degrees, per-pair minimum, triangles per pair, triangles); a finite minimum is met within the
# 1e-9 degrees of the comparison with the device (an exact loop closes to rounding, not to 0.0)
EDGE_ANSWERS = {
    "path": ([1, 1, 1], [INF] * 3, [0, 0, 0], 0),
    "star": ([1, 1, 1], [INF] * 3, [0, 0, 0], 0),
    "four-cycle": ([1, 1, 1, 1], [INF] * 4, [0, 0, 0, 0], 0),
    "exact-triangle": ([0, 0, 0], [0.0] * 3, [1, 1, 1], 1),
    "half-turn": ([1, 1, 1], [180.0] * 3, [1, 1, 1], 1),
    # (0, 1) has the NaN: its two triangles validate nothing; the other five pairs lie in one sound triangle each
    "nan-pair": ([1, 0, 0, 0, 0, 0], [INF, 0.0, 0.0, 0.0, 0.0, 0.0], [2, 2, 2, 2, 2, 2], 4),
    "unnamed-views": ([0, 0, 0], [0.0] * 3, [1, 1, 1], 1),
    "equal-components": ([0] * 6, [0.0] * 6, [1] * 6, 2),
    "small-component": ([1, 0, 0, 0], [INF, 0.0, 0.0, 0.0], [0, 1, 1, 1], 1),
}
# name: (removed pairs, removed views, component)
COMPONENT_ANSWERS = {
    "path": ([0] * 3, [0] * 4, [0] * 4),
    "unnamed-views": ([0] * 3, [0] * 8, [-1, 1, -1, -1, 1, -1, 1, -1]),
    "equal-components": ([1, 1, 1, 0, 0, 0], [0, 1, 0, 1, 0, 1], [0, 1, 0, 1, 0, 1]),   # {0, 2, 4} holds the smallest view
    "small-component": ([1, 0, 0, 0], [1, 1, 0, 0, 0], [0, 0, 2, 2, 2]),
}


def check_edge_answer(name, got, threshold=4.0):
    """`got` (the restatement's or the device's dict) against the hand-written answer."""
    removed, minimum, count, total = EDGE_ANSWERS[name]
    if threshold == 4.0:
        assert got["removed"].astype(int).tolist() == removed, name
    assert got["triangles_per_pair"].tolist() == count and int(got["num_triangles"]) == total, name
    for m, want in zip(got["min_loop_error_degrees"], minimum):
        if want == INF:
            assert m == INF, name
        else:
            assert 0.0 <= m and abs(m - want) < 1e-9, (name, m)


@pytest.mark.parametrize("name", list(EDGE_ANSWERS))
def test_restatement_on_the_edge_scenes(name):
    s = ref.edge_scenes()[name]
    assert set(EDGE_ANSWERS) == set(ref.edge_scenes())
    check_edge_answer(name, s["ref"][4.0])
    if name == "half-turn":
        assert not s["ref"][181.0]["removed"].any()


@pytest.mark.parametrize("name", list(COMPONENT_ANSWERS))
def test_restated_components_on_the_edge_scenes(name):
    s = ref.edge_scenes()[name]
    c = ref.components(s["n"], s["pairs"])
    pairs, views, comp = COMPONENT_ANSWERS[name]
    assert c["removed_pairs"].astype(int).tolist() == pairs
    assert c["removed_views"].astype(int).tolist() == views
    assert c["component"].tolist() == comp


# ------------------------------------------------------------------------- theia_hip_remove_disconnected_view_pairs
def split_scene():
    """The dense scene's pairs, cut into three parts of 50, 50 and 20 views with the indices interleaved, and 7 views more
    that no pair names: two components of equal size, of which the one holding view 0 stays."""
    d = ref.dense_scene()
    part = np.array([0 if v < 50 else (1 if v < 100 else 2) for v in range(d["n"])])
    keep = part[d["pairs"][:, 0]] == part[d["pairs"][:, 1]]
    new = np.concatenate([np.arange(0, 100, 2), np.arange(1, 100, 2), np.arange(100, 120)]) + 3   # views 0 .. 2 stay unnamed
    new[0] = 0                                                                                      # ... but for view 0
    pairs = np.ascontiguousarray(new[d["pairs"][keep]].astype(np.int32))
    return 127, pairs


def component_cases():
    cases = [(s["name"], s["n"], s["pairs"]) for s in ref.all_scenes()]
    n, pairs = split_scene()
    return cases + [("split", n, pairs)]


@pytest.mark.parametrize("name,n,pairs", component_cases(), ids=[c[0] for c in component_cases()])
def test_remove_disconnected_equals_the_restatement(name, n, pairs):
    rc, removed_pairs, removed_views, component = global_pose.remove_disconnected_pairs(n, pairs)
    want = ref.components(n, pairs)
    assert rc == 0
    assert np.array_equal(removed_pairs, want["removed_pairs"])
    assert np.array_equal(removed_views, want["removed_views"])
    assert np.array_equal(component, want["component"])
    if name in COMPONENT_ANSWERS:
        assert removed_views.astype(int).tolist() == COMPONENT_ANSWERS[name][1]
        assert component.tolist() == COMPONENT_ANSWERS[name][2]
    # the component labels: the smallest view of the component, -1 exactly for the views no pair names
    named = np.zeros(n, bool)
    named[pairs.ravel()] = True
    assert np.array_equal(component == -1, ~named) and not removed_views[~named].any()
    assert all(component[component[v]] == component[v] <= v for v in np.flatnonzero(named))
    assert np.array_equal(component[pairs[:, 0]], component[pairs[:, 1]])
    if name == "split":
        sizes = np.bincount(component[named])
        assert sorted(sizes[sizes > 0].tolist()) == [20, 50, 50]
        assert not removed_views[0] and int(removed_views.sum()) == 70 and removed_pairs.any() and not removed_pairs.all()


def _call(n, pairs, views=True, out_pairs=True):
    pairs = None if pairs is None else np.ascontiguousarray(pairs, dtype=np.int32)
    E = 0 if pairs is None else len(pairs)
    removed_pairs = np.full(max(E, 1), 0x5A, dtype=np.uint8)
    removed_views = np.full(max(n, 1), 0x5A, dtype=np.uint8)
    component = np.full(max(n, 1), -77, dtype=np.int32)
    rc = capi.lib().theia_hip_remove_disconnected_view_pairs(
        n, E, capi.ptr(pairs, C.c_int32), capi.ptr(removed_pairs if out_pairs else None, C.c_uint8),
        capi.ptr(removed_views if views else None, C.c_uint8), capi.ptr(component, C.c_int32))
    untouched = bool(np.all(removed_pairs == 0x5A) and np.all(removed_views == 0x5A) and np.all(component == -77))
    return rc, untouched


def test_remove_disconnected_refusals_and_empty_list():
    p = ref.reference_scene(5)["pairs"]
    n = 10
    assert _call(n, p) == (0, False)
    bad = p.copy(); bad[4, 1] = n
    assert _call(n, bad) == (INVALID, True)
    bad = p.copy(); bad[4, 0] = -1
    assert _call(n, bad) == (INVALID, True)
    bad = p.copy(); bad[4, 1] = bad[4, 0]
    assert _call(n, bad) == (INVALID, True)          # a self-pair
    bad = p.copy(); bad[20] = bad[3]
    assert _call(n, bad) == (INVALID, True)          # the same pair twice
    bad = p.copy(); bad[20] = bad[3][::-1]
    assert _call(n, bad) == (INVALID, True)          # ... and reversed: the same unordered pair
    assert _call(n, p, views=False) == (INVALID, True)
    assert _call(n, p, out_pairs=False) == (INVALID, True)
    removed = np.zeros(len(p), np.uint8)
    views = np.zeros(n, np.uint8)
    assert capi.lib().theia_hip_remove_disconnected_view_pairs(n, len(p), None, capi.ptr(removed, C.c_uint8),
                                                               capi.ptr(views, C.c_uint8), None) == INVALID
    assert b"null" in capi.lib().theia_hip_last_error()
    # no pairs: accepted, nothing is removed
    rc, removed_pairs, removed_views, component = global_pose.remove_disconnected_pairs(6, np.zeros((0, 2), np.int32))
    assert rc == 0 and removed_pairs.shape == (0,) and not removed_views.any() and np.all(component == -1)
    assert _call(0, None)[0] == 0


# ----------------------------------------------------------------------------------------------------- the mirror
def test_pytheia_names_and_symbols():
    for name in ("FilterViewGraphCyclesByRotation", "RemoveDisconnectedViewPairs"):
        assert getattr(sfm, name) is getattr(global_pose, name)
    for name in ("theia_hip_filter_view_graph_cycles_by_rotation", "theia_hip_remove_disconnected_view_pairs"):
        assert name in capi.EXPORTED_SYMBOLS and hasattr(capi.lib(), name)


def view_pairs_dict(ids, pairs, rotation_2=None):
    """{(id1, id2): TwoViewInfo} of pairs over view indices, renamed by ids[index]."""
    out = {}
    for e, (a, b) in enumerate(pairs):
        info = twoview.TwoViewInfo()
        if rotation_2 is not None:
            info.rotation_2 = np.array(rotation_2[e])
        out[(int(ids[a]), int(ids[b]))] = info
    return out


def test_remove_disconnected_view_pairs_on_the_dict():
    # ids that are no indices: 'smallest view index' means smallest view id
    ids = np.array([70, 11, 52, 13, 34, 95])
    s = ref.edge_scenes()["equal-components"]            # index components {1, 3, 5} and {0, 2, 4}
    vp = view_pairs_dict(ids, s["pairs"])
    gone = sfm.RemoveDisconnectedViewPairs(vp)
    assert gone == {70, 52, 34}                          # id 11 is the smallest: {11, 13, 95} stays
    assert set(vp) == {(11, 13), (13, 95), (11, 95)}
    s = ref.edge_scenes()["small-component"]
    vp = view_pairs_dict(ids, s["pairs"])
    assert sfm.RemoveDisconnectedViewPairs(vp) == {70, 11} and set(vp) == {(52, 13), (13, 34), (52, 34)}
    vp = view_pairs_dict(ids, ref.edge_scenes()["path"]["pairs"])
    assert sfm.RemoveDisconnectedViewPairs(vp) == set() and len(vp) == 3
    assert sfm.RemoveDisconnectedViewPairs({}) == set()
