"""CPU: the NONLINEAR rotation stage without a device -- the torch restatement (tests/nonlinear_rotation_ref.py) against
finite differences of its own residual and against the behaviour measured for it (iteration counts, stopping rules,
margins, the Cholesky / LU / permutation spread), OrientationsFromMaximumSpanningTree, and the paths of the mirror and
of theia_hip_nonlinear_rotations that return before the device is touched."""
import ctypes

import numpy as np
import pytest
import torch

from pytheiasfm_amd import _capi as capi
from pytheiasfm_amd import global_pose, sfm
from pytheiasfm_amd.twoview import TwoViewInfo
from tests import nonlinear_rotation_ref as ref
from tests import rotation_scenes as rs
from tests.rotation_averaging_ref import aa_to_R

# (views, pairs, noise degrees, outlier fraction, seed) -> iterations; all stop on the function tolerance
SCENES = {(4, 6, 1.0, 0.0, 1): 3, (21, 80, 2.0, 0.0, 1): 4, (22, 80, 2.0, 0.1, 2): 4, (43, 300, 2.0, 0.1, 3): 4,
          (100, 800, 2.0, 0.1, 1): 4}
_solved = {}


def solved(spec):
    if spec not in _solved:
        s = rs.make_scene(*spec)
        _solved[spec] = (s, ref.solve(s["init"], s["edges"], s["rel"]))
    return _solved[spec]


def _fd(w1, w2, rel, h=1e-6):
    J = np.zeros((3, 6))
    x = np.concatenate([w1, w2])
    for k in range(6):
        p, m = x.copy(), x.copy()
        p[k] += h; m[k] -= h
        J[:, k] = (ref.residual(torch.tensor(p[:3]), torch.tensor(p[3:]), torch.tensor(rel)).numpy()
                   - ref.residual(torch.tensor(m[:3]), torch.tensor(m[3:]), torch.tensor(rel)).numpy()) / (2.0 * h)
    return J


@pytest.mark.parametrize("case", ["zero_w1", "zero_residual", "generic", "beyond_120_degrees"])
def test_restatement_jacobian_against_central_differences(case):
    rng = np.random.default_rng(5)
    w1, w2, rel = rng.uniform(-0.4, 0.4, 3), rng.uniform(-0.4, 0.4, 3), rng.uniform(-0.4, 0.4, 3)
    if case == "zero_w1":
        w1 = np.zeros(3)
    elif case == "zero_residual":                      # rel = the rotation from w1 to w2, up to rounding
        w1 = np.zeros(3); rel = w2.copy()
    elif case == "beyond_120_degrees":                 # trace < 0: a largest-diagonal branch of the quaternion
        rel = np.array([2.6, 0.3, -0.2])
    r = ref.residual(torch.tensor(w1), torch.tensor(w2), torch.tensor(rel)).numpy()
    if case == "zero_residual":
        assert np.abs(r).max() < 1e-15
    j1, j2 = (t.numpy()[0] for t in ref._jac(torch.tensor(w1[None]), torch.tensor(w2[None]), torch.tensor(rel[None])))
    fd = _fd(w1, w2, rel)
    # central differences with h = 1e-6: truncation ~ h^2 |r'''| ~ 1e-12, rounding ~ eps |r| / h ~ 1e-9 at |r| ~ 3
    assert np.all(np.isfinite(j1)) and np.all(np.isfinite(j2))
    assert np.abs(np.hstack([j1, j2]) - fd).max() < 5e-9


def test_noise_free_scene_stops_before_any_iteration():
    s = rs.make_scene(4, 6, 0.0, 0.0, 1)
    o = ref.solve(s["init"], s["edges"], s["rel"])
    assert o["iterations"] == 0 and o["term"] == ref.TERM_GRADIENT
    assert o["cost"] < 1e-28 and np.array_equal(o["x"], s["init"])


@pytest.mark.parametrize("spec", list(SCENES))
def test_scene_behaviour(spec):
    s, o = solved(spec)
    assert o["iterations"] == SCENES[spec] and o["term"] == ref.TERM_FUNCTION
    assert o["successful"] == o["iterations"] - 1 and o["unsuccessful"] == 0 and o["invalid"] == 0
    assert o["margin"] > 0.5                             # measured: 0.507 .. 0.911
    e0, e1 = rs.aligned_errors_deg(s["init"], s["gt"]).max(), rs.aligned_errors_deg(o["x"], s["gt"]).max()
    assert e1 < e0
    if spec[0] > 4:
        assert 5.0 < e0 < 12.0 and 1.3 < e1 < 2.3       # measured: 5.1 .. 11.2 degrees -> 1.44 .. 2.22 degrees


def test_rounding_spread_cholesky_lu_permutation():
    spec = (43, 300, 2.0, 0.1, 3)
    s, o = solved(spec)
    lu = ref.solve(s["init"], s["edges"], s["rel"], linear="lu")
    assert lu["iterations"] == o["iterations"]
    assert rs.angle_between(lu["x"], o["x"]).max() < 1e-12
    perm = np.random.default_rng(0).permutation(spec[0])        # view v becomes perm[v]
    init = np.zeros_like(s["init"]); init[perm] = s["init"]
    p = ref.solve(init, perm[s["edges"]], s["rel"])
    assert p["iterations"] == o["iterations"]
    assert rs.angle_between(p["x"][perm], o["x"]).max() < 1e-12


def test_rejected_step_scene():
    s = rs.make_scene(10, 25, 5.0, 0.4, seed=19)
    x0 = np.random.default_rng(119).uniform(-2.5, 2.5, (10, 3))
    o = ref.solve(x0, s["edges"], s["rel"], robust_loss_width=0.01)
    assert (o["iterations"], o["successful"], o["unsuccessful"], o["invalid"]) == (34, 26, 7, 0)
    assert [k for k, t in enumerate(o["trace"]) if t[4] == 0][:7] == list(range(11, 18))
    assert o["term"] == ref.TERM_FUNCTION and 9e7 < o["radius"] < 1e8 and 0.1 < o["margin"] < 0.13


def test_fixed_views_keep_their_bits_and_take_no_columns():
    s, _ = solved((21, 80, 2.0, 0.0, 1))
    fixed = np.zeros(21, dtype=bool); fixed[[0, 7]] = True
    o = ref.solve(s["init"], s["edges"], s["rel"], fixed=fixed)
    assert np.array_equal(o["x"][fixed], s["init"][fixed]) and not np.array_equal(o["x"][~fixed], s["init"][~fixed])


# ---- OrientationsFromMaximumSpanningTree

def _pairs(edges, rel, weights):
    out = {}
    for (a, b), r, w in zip(edges, rel, weights):
        info = TwoViewInfo()
        info.rotation_2 = np.array(r, dtype=np.float64)
        info.num_verified_matches = int(w)
        out[(int(a), int(b))] = info
    return out


def _tree_edges(pairs, orientations, tol=1e-12):
    """the pairs that the orientations satisfy exactly: the tree, when the relative rotations are noisy"""
    tree = []
    for (a, b), info in pairs.items():
        if a in orientations and b in orientations:
            Ra, Rb, Rr = (aa_to_R(np.asarray(v)[None])[0] for v in (orientations[a], orientations[b], info.rotation_2))
            if np.abs(Rb @ Ra.T - Rr).max() < tol:
                tree.append((a, b))
    return sorted(tree)


def test_spanning_tree_distinct_weights():
    s = rs.make_scene(12, 30, 2.0, 0.0, 3)
    w = np.random.default_rng(1).permutation(30) + 10
    pairs = _pairs(s["edges"] + 5, s["rel"], w)                               # ids 5 .. 16
    pairs.update(_pairs([(40, 41), (41, 42)], [[0.1, 0, 0], [0, 0.2, 0]], [999, 998]))   # a smaller component
    o = global_pose.OrientationsFromMaximumSpanningTree(pairs)
    assert sorted(o) == list(range(5, 17)) and np.array_equal(o[5], np.zeros(3))
    tree = _tree_edges(pairs, o)
    assert len(tree) == 11
    # the maximum spanning tree by a second route: Prim from the root on the component's pairs
    comp = {p: i for p, i in pairs.items() if p[0] < 40}
    seen, prim = {5}, []
    while len(seen) < 12:
        best = max((p for p in comp if (p[0] in seen) != (p[1] in seen)), key=lambda p: comp[p].num_verified_matches)
        prim.append(best); seen.update(best)
    assert tree == sorted(prim)
    assert sfm.OrientationsFromMaximumSpanningTree is global_pose.OrientationsFromMaximumSpanningTree
    assert global_pose.OrientationsFromMaximumSpanningTree({}) == {}


def test_spanning_tree_rules_under_ties_and_relabelling():
    # a 4-cycle of equal weights with noisy (inconsistent) rotations: the tree drops the pair with the largest ids
    rng = np.random.default_rng(2)
    edges = [(1, 2), (2, 3), (3, 4), (1, 4)]
    rel = rng.uniform(-0.3, 0.3, (4, 3))
    pairs = _pairs(edges, rel, [7, 7, 7, 7])
    o = global_pose.OrientationsFromMaximumSpanningTree(pairs)
    assert np.array_equal(o[1], np.zeros(3))
    assert _tree_edges(pairs, o) == [(1, 2), (1, 4), (2, 3)]
    # the order of the dict does not matter
    back = global_pose.OrientationsFromMaximumSpanningTree(dict(reversed(list(pairs.items()))))
    assert all(np.array_equal(o[v], back[v]) for v in o)
    # relabelled ids (order reversed: 1, 2, 3, 4 -> 40, 30, 20, 10): the rules follow the new ids
    m = {1: 40, 2: 30, 3: 20, 4: 10}
    moved = {}
    for (a, b), info in pairs.items():
        flipped = TwoViewInfo()
        flipped.rotation_2 = -info.rotation_2              # the pair is stored under (smaller, larger): b -> a
        flipped.num_verified_matches = info.num_verified_matches
        moved[(m[b], m[a])] = flipped
    o2 = global_pose.OrientationsFromMaximumSpanningTree(moved)
    assert np.array_equal(o2[10], np.zeros(3))
    assert _tree_edges(moved, o2) == [(10, 20), (10, 40), (20, 30)]
    # equal sizes: the component with the smallest view id
    two = _pairs([(8, 9), (3, 4)], [[0.1, 0, 0], [0, 0.1, 0]], [5, 50])
    assert sorted(global_pose.OrientationsFromMaximumSpanningTree(two)) == [3, 4]


# ---- the mirror and the C entry point, without a device

def test_names_and_struct_sizes():
    assert sfm.NonlinearRotationEstimator is global_pose.NonlinearRotationEstimator
    assert sfm.NonlinearRotationEstimatorOptions is global_pose.NonlinearRotationEstimatorOptions
    assert global_pose.GlobalRotationEstimatorType.NONLINEAR == 1
    assert ctypes.sizeof(capi.NonlinearRotationOptions) == 2 * 4 + 5 * 8
    assert ctypes.sizeof(capi.NonlinearRotationSummary) == 8 * 4 + 5 * 8
    o = global_pose.NonlinearRotationEstimatorOptions().to_c()
    assert (o.max_num_iterations, o.robust_loss_width, o.function_tolerance, o.gradient_tolerance, o.parameter_tolerance,
            o.max_trust_region_radius) == (200, 0.1, 1e-6, 1e-10, 1e-8, 1e16)
    with pytest.raises(ValueError):
        global_pose.nonlinear_rotations(np.zeros((3, 3)), [[0, 1], [1, 2]], np.zeros((1, 3)))
    with pytest.raises(ValueError):
        global_pose.nonlinear_rotations(np.zeros((3, 3)), [[0, 1]], np.zeros((1, 3)), fixed=[True])


def _refused(aa, edges, rel, fixed=None, **opts):
    o = global_pose.NonlinearRotationEstimatorOptions()
    for k, v in opts.items():
        setattr(o, k, v)
    before = np.array(aa, dtype=np.float64)
    rc, out, summ = global_pose.nonlinear_rotations(before, edges, rel, fixed, o)
    assert rc == capi.THEIA_HIP_ERR_INVALID_ARGUMENT
    assert np.array_equal(out, before)
    assert bytes(summ) == bytes(capi.NonlinearRotationSummary())


def test_refusals_before_the_device_is_touched():
    aa = np.random.default_rng(0).uniform(-1, 1, (3, 3))
    e, r = np.array([[0, 1], [1, 2]], dtype=np.int32), np.zeros((2, 3))
    _refused(aa, np.zeros((0, 2), dtype=np.int32), np.zeros((0, 3)))
    _refused(aa, [[0, 3], [1, 2]], r)
    _refused(aa, [[0, 1], [-1, 2]], r)
    _refused(aa, [[0, 1], [2, 2]], r)
    for bad in (0.0, -0.1, np.inf, np.nan):
        _refused(aa, e, r, robust_loss_width=bad)
        _refused(aa, e, r, max_trust_region_radius=bad)
    for name in ("function_tolerance", "gradient_tolerance", "parameter_tolerance"):
        for bad in (-1e-6, np.inf, np.nan):
            _refused(aa, e, r, **{name: bad})
    _refused(aa, e, r, max_num_iterations=-1)


def _info(r):
    info = TwoViewInfo()
    info.rotation_2 = np.array(r, dtype=np.float64)
    return info


def test_mirror_empty_inputs_and_skipped_pairs(monkeypatch):
    est = sfm.NonlinearRotationEstimator()
    assert est.options.robust_loss_width == 0.1 and sfm.NonlinearRotationEstimator(0.25).options.robust_loss_width == 0.25
    given = {3: np.array([0.1, 0.2, 0.3])}
    for pairs, orientations in (({}, given), ({(3, 9): _info([0, 0, 0.1])}, {}), ({(3, 9): _info([0, 0, 0.1])}, given)):
        out = est.EstimateRotations(pairs, orientations)    # no pair, no orientation, no pair with both orientations
        assert est.last_success is False and isinstance(est.last_summary, capi.NonlinearRotationSummary)
        assert sorted(out) == sorted(orientations) and all(np.array_equal(out[v], orientations[v]) for v in out)
    calls = []

    def fake(aa, edges, rel, fixed=None, options=None, want_trace=False):
        calls.append((np.array(aa), np.array(edges), np.array(rel), fixed, options))
        return 0, np.array(aa) + 1.0, capi.NonlinearRotationSummary()

    monkeypatch.setattr(global_pose, "nonlinear_rotations", fake)
    orientations = {30: np.array([0.1, 0, 0]), 10: np.array([0, 0.2, 0]), 20: np.array([0, 0, 0.3])}
    pairs = {(10, 20): _info([1, 0, 0]), (20, 99): _info([2, 0, 0]), (30, 20): _info([3, 0, 0])}
    keep = {v: r.copy() for v, r in orientations.items()}
    out = est.EstimateRotations(pairs, orientations)
    assert est.last_success is True and len(calls) == 1
    aa, edges, rel, fixed, options = calls[0]
    assert fixed is None and options is est.options
    assert edges.tolist() == [[1, 2], [0, 2]] and rel[:, 0].tolist() == [1.0, 3.0]       # the pair naming view 99 is skipped
    assert all(np.array_equal(orientations[v], keep[v]) for v in keep)                  # the input is not modified
    assert sorted(out) == [10, 20, 30] and np.array_equal(out[10], keep[10] + 1.0)
