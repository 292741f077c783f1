"""GPU: theia_hip_filter_view_graph_cycles_by_rotation (csrc/view_graph_pruning.hip) against the sequential numpy
restatement (tests/view_graph_pruning_ref.py), never against a second run of the device code except where byte-identity
of two runs is the point.

Every scene is compared at every threshold it carries, and its builder has asserted of the restatement alone that no
finite per-pair minimum lies within 1e-6 degrees of one: the verdicts, the triangle counts and the places of +inf are
compared exactly and for every pair.  The finite minima are compared to MIN_TOL = 1e-9 degrees.  That bound is no
measurement: the entries of a product of three rotation matrices carry a few ulp, and the angle goes through atan2 of
the quaternion parts, which is well conditioned everywhere, so an honest difference is about 1e-13 degrees with or
without fused multiply-adds, while a transposed or mis-picked matrix is off by degrees."""
import ctypes as C

import numpy as np
import pytest

from pytheiasfm_amd import _capi as capi
from pytheiasfm_amd import global_pose, sfm
from tests import view_graph_pruning_ref as ref
from tests.test_view_graph_pruning import check_edge_answer, view_pairs_dict

pytestmark = pytest.mark.gpu

INVALID = capi.THEIA_HIP_ERR_INVALID_ARGUMENT
MIN_TOL = 1e-9   # degrees
WANT = ("min_loop_error_degrees", "triangles_per_pair", "num_triangles")
CASES = [(s["name"], t) for s in ref.all_scenes() for t in s["thresholds"]]
BY_NAME = {s["name"]: s for s in ref.all_scenes()}


def run(s, threshold, pairs=None, rotation_2=None):
    rc, removed, got = global_pose.filter_cycles_by_rotation(
        s["n"], s["pairs"] if pairs is None else pairs, s["rotation_2"] if rotation_2 is None else rotation_2, threshold, want=WANT)
    assert rc == 0
    got["removed"] = removed
    return got


def compare(got, want):
    """The device's outputs against the restatement's; returns the largest difference of the finite minima."""
    assert np.array_equal(got["removed"], want["removed"])
    assert np.array_equal(got["triangles_per_pair"], want["triangles_per_pair"])
    assert got["num_triangles"] == want["num_triangles"]
    g, w = got["min_loop_error_degrees"], want["min_loop_error_degrees"]
    assert np.array_equal(np.isinf(g), np.isinf(w)) and not np.isnan(g).any() and (g >= 0.0).all()
    fin = np.isfinite(w)
    worst = float(np.abs(g[fin] - w[fin]).max()) if fin.any() else 0.0
    print(f"largest difference of the finite minima: {worst:.3e} degrees")
    assert worst <= MIN_TOL
    return worst


@pytest.mark.parametrize("name,threshold", CASES, ids=[f"{n}-{t}" for n, t in CASES])
def test_equals_the_restatement(name, threshold):
    s = BY_NAME[name]
    got = run(s, threshold)
    compare(got, s["ref"][threshold])
    if name in ref.edge_scenes():
        check_edge_answer(name, got, threshold)


@pytest.mark.parametrize("name", ["reference-15", "hub", "dense", "nan-pair"])
def test_orientation_of_a_stored_pair_does_not_matter(name):
    """Every pair stored the other way round with its rotation_2 negated (the rotation of that orientation)."""
    s = BY_NAME[name]
    t = s["thresholds"][0]
    flipped = run(s, t, pairs=np.ascontiguousarray(s["pairs"][:, ::-1]), rotation_2=-s["rotation_2"])
    compare(flipped, s["ref"][t])
    # ... and only the pairs that were ascending, so that both orders occur in every scene
    asc = s["pairs"][:, 0] < s["pairs"][:, 1]
    pairs, rot = s["pairs"].copy(), s["rotation_2"].copy()
    pairs[asc] = pairs[asc][:, ::-1]
    rot[asc] = -rot[asc]
    assert (pairs[:, 0] > pairs[:, 1]).all()
    compare(run(s, t, pairs=pairs, rotation_2=rot), s["ref"][t])


def test_thresholds_that_nothing_is_below():
    s = BY_NAME["exact-triangle"]
    for t in (0.0, -1.0, float("nan")):
        got = run(s, t)
        assert got["removed"].all() and got["num_triangles"] == 1 and (got["min_loop_error_degrees"] < MIN_TOL).all()
    d = BY_NAME["dense"]
    for t in (-1e-300, float("nan")):
        got = run(d, t)
        assert got["removed"].all()
        assert np.array_equal(got["triangles_per_pair"], d["ref"][4.0]["triangles_per_pair"])
    assert not run(s, float("inf"))["removed"].any()


def test_nan_rotation_validates_nothing():
    s = BY_NAME["nan-pair"]
    got = run(s, 4.0)
    assert got["removed"].tolist() == [True] + [False] * 5          # the NaN pair goes, its neighbours stay by their other triangles
    assert got["min_loop_error_degrees"][0] == np.inf and got["triangles_per_pair"][0] == 2
    # without the sound triangles (0, 2, 3) and (1, 2, 3), i.e. without the pair (2, 3), nothing validates the neighbours
    got = run(s, 4.0, pairs=s["pairs"][:5], rotation_2=s["rotation_2"][:5])
    assert got["removed"].all() and np.isinf(got["min_loop_error_degrees"]).all() and got["num_triangles"] == 2


def test_two_runs_are_byte_identical():
    d = BY_NAME["dense"]
    a, b = run(d, 4.0), run(d, 4.0)
    for k in ("removed", "min_loop_error_degrees", "triangles_per_pair"):
        assert a[k].tobytes() == b[k].tobytes()
    assert a["num_triangles"] == b["num_triangles"]


def _call(n, pairs, rot, removed_ptr=True):
    pairs = None if pairs is None else np.ascontiguousarray(pairs, dtype=np.int32)
    E = 0 if pairs is None else len(pairs)
    removed = np.full(max(E, 1), 0x5A, dtype=np.uint8)
    minimum = np.full(max(E, 1), -7.0)
    count = np.full(max(E, 1), -7, dtype=np.int32)
    total = np.full(1, -7, dtype=np.int64)
    rc = capi.lib().theia_hip_filter_view_graph_cycles_by_rotation(
        n, E, capi.ptr(pairs, C.c_int32), capi.ptr(rot, C.c_double), 4.0, capi.ptr(removed if removed_ptr else None, C.c_uint8),
        capi.ptr(minimum, C.c_double), capi.ptr(count, C.c_int32), capi.ptr(total, C.c_int64))
    untouched = bool(np.all(removed == 0x5A) and np.all(minimum == -7.0) and np.all(count == -7) and total[0] == -7)
    return rc, untouched


def test_refusals_and_empty_list():
    s = ref.reference_scene(5)
    n, p, rot = s["n"], s["pairs"], s["rotation_2"]
    assert _call(n, p, rot) == (0, False)
    bad = p.copy(); bad[4, 1] = n
    assert _call(n, bad, rot) == (INVALID, True)
    bad = p.copy(); bad[4, 0] = -1
    assert _call(n, bad, rot) == (INVALID, True)
    bad = p.copy(); bad[4, 1] = bad[4, 0]
    assert _call(n, bad, rot) == (INVALID, True)          # a self-pair
    bad = p.copy(); bad[20] = bad[3]
    assert _call(n, bad, rot) == (INVALID, True)          # the same pair twice
    bad = p.copy(); bad[20] = bad[3][::-1]
    assert _call(n, bad, rot) == (INVALID, True)          # ... and reversed: the same unordered pair
    assert _call(n, p, None) == (INVALID, True)
    assert _call(n, p, rot, removed_ptr=False) == (INVALID, True)
    removed = np.full(len(p), 0x5A, dtype=np.uint8)
    assert capi.lib().theia_hip_filter_view_graph_cycles_by_rotation(
        n, len(p), None, capi.ptr(rot, C.c_double), 4.0, capi.ptr(removed, C.c_uint8), None, None, None) == INVALID
    assert np.all(removed == 0x5A)
    # no pairs: accepted, nothing launched
    assert _call(n, None, None)[0] == 0
    rc, removed, got = global_pose.filter_cycles_by_rotation(n, np.zeros((0, 2), np.int32), np.zeros((0, 3)), 4.0, want=WANT)
    assert rc == 0 and removed.shape == (0,) and got["num_triangles"] == 0
    # only the verdicts asked for
    rc, removed, got = global_pose.filter_cycles_by_rotation(n, p, rot, 4.0)
    assert rc == 0 and got == {} and np.array_equal(removed, s["bad"])


def test_end_to_end_on_the_dict():
    """The reference scene with 15 bad pairs and, on three further views, an isolated sound triangle: the filter deletes the
    15, then the pruning returns the three views and deletes their pairs."""
    s = ref.reference_scene(15)
    ids = 100 + 7 * np.arange(13)                  # view ids that are no indices; the triangle has the largest
    extra = [(10, 11), (10, 12), (11, 12)]
    pairs = np.concatenate([s["pairs"], np.array(extra, dtype=np.int32)])
    rot = np.concatenate([s["rotation_2"], np.array(ref.exact_rotations(13, extra))])
    vp = view_pairs_dict(ids, pairs, rot)
    assert len(vp) == 48
    assert sfm.FilterViewGraphCyclesByRotation(4.0, vp) == 15
    good = [(int(ids[a]), int(ids[b])) for (a, b), bad in zip(s["pairs"], s["bad"]) if not bad]
    triangle = [(int(ids[a]), int(ids[b])) for a, b in extra]
    assert set(vp) == set(good) | set(triangle)
    assert sfm.RemoveDisconnectedViewPairs(vp) == {int(ids[10]), int(ids[11]), int(ids[12])}
    assert set(vp) == set(good)
