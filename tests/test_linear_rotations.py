"""CPU: the LINEAR rotation stage without a device -- the numpy restatement (tests/linear_rotation_ref.py) against ground
truth, the scene conditions the GPU tests rest on, the step-by-step restatement against the eigh one, every refusal of
theia_hip_linear_rotations (all of them return before the device is touched), and the Python class's bookkeeping."""
import types

import numpy as np
import pytest

from pytheiasfm_amd import _capi as capi, global_pose, sfm
from tests import linear_rotation_ref as ref
from tests import linear_rotation_scenes as ls
from tests import rotation_scenes as rs

EPS = np.finfo(float).eps


@pytest.mark.parametrize("name", list(ls.GT_BOUND_DEG))
def test_reference_recovers_ground_truth(name):
    s, r, d = ls.scene(name)
    for which, res in (("eigh", r), ("steps", d)):
        err = rs.aligned_errors_deg(res["orientations"], s["gt"][res["views"]]).max()
        print(f"{name} {which}: aligned error {err:.3e} degrees, bound {ls.GT_BOUND_DEG[name]}")
        assert err <= ls.GT_BOUND_DEG[name]


@pytest.mark.parametrize("name", ls.SCENES)
def test_scene_conditions(name):
    s, r, d = ls.scene(name)
    assert ls.connected(s["n"], s["edges"])
    assert len(r["views"]) == s["n"]                       # every view of these scenes has an edge
    w = r["eigenvalues"]
    n3 = len(w)
    assert n3 == 3 * s["n"]
    if n3 > 3:
        print(f"{name}: lambda_3 / lambda_4 = {w[2] / w[3]:.3e}, iterations {d['iterations']}")
        assert w[2] / w[3] <= 0.2                          # the subspace iteration gains a factor of 5 or more per step
    if name in ls.NOISE_FREE:
        assert np.abs(w[:3]).max() <= 64 * n3 * EPS * w[-1]   # three null vectors, to rounding
        assert w[3] > 1e-3 * w[-1]                            # and only three
    assert d["converged"] and 2 <= d["iterations"] <= 16
    assert d["shift"] == (n3 * EPS) * r["M"].diagonal().max()


def test_scene_shapes():
    assert [3 * ls.graph(k)["n"] for k in ("v21", "v22", "v43", "v700")] == [63, 66, 129, 2100]
    s = ls.graph("v60dup")
    assert len(s["edges"]) == 550
    pairs = [tuple(e) for e in s["edges"]]
    assert len(set(pairs)) < len(pairs) and any((b, a) in set(pairs) for a, b in pairs)   # repeated and reversed
    ring = ls.graph("ring24")
    assert len(ring["edges"]) == 48 and np.isclose(np.degrees(ring["gt"][12, 1]), 180.0)
    assert np.degrees(np.linalg.norm(ring["rel"], axis=1)).max() < 35.0   # the relative rotations stay small
    assert ls.graph("v300out")["outliers"].sum() == 300


@pytest.mark.parametrize("name", ls.SCENES)
def test_steps_equal_eigh(name):
    _, r, d = ls.scene(name)
    angle = ref.gauge_free_angles(d["orientations"], r["orientations"]).max()
    w = r["eigenvalues"]
    print(f"{name}: {angle:.3e} rad, eigenvalue difference {np.abs(d['eigenvalues'] - w[:3]).max() / w[-1]:.3e} lambda_max")
    assert angle <= 1e-9
    assert np.abs(d["eigenvalues"] - w[:3]).max() <= 1e-9 * w[-1]


def test_build_M_is_the_reference_matrix():
    """Block by block, against the description: symmetric, degree on the diagonal, -R_e^T at (i, j)."""
    s = ls.graph("tiny1")
    M, views = ref.build_M(s["n"], s["edges"], s["rel"])
    assert list(views) == [0, 1, 2, 3] and np.array_equal(M, M.T)
    deg = np.bincount(s["edges"].ravel(), minlength=4)
    for v in range(4):
        assert np.array_equal(M[3 * v:3 * v + 3, 3 * v:3 * v + 3], deg[v] * np.eye(3))
    (i, j), Re = s["edges"][0], ref.aa_to_R(s["rel"][:1])[0]
    assert np.array_equal(M[3 * i:3 * i + 3, 3 * j:3 * j + 3], -Re.T)
    # the ground truth spans the null space on noise-free input: M [R_0; R_1; ...] = 0
    s0 = ls.graph("tiny0")
    M0, _ = ref.build_M(s0["n"], s0["edges"], s0["rel"])
    assert np.abs(M0 @ ref.aa_to_R(s0["gt"]).reshape(-1, 3)).max() <= 64 * EPS


def test_start_block():
    X = ref.start_block(5)
    assert X.shape == (5, 3) and X[0, 0] == ((2654435761 >> 8) * 2.0 ** -23 - 1.0)
    assert X[1, 2] == ((((6 * 2654435761) & 0xFFFFFFFF) >> 8) * 2.0 ** -23 - 1.0)
    assert np.all(X >= -1.0) and np.all(X < 1.0)


# ---- refusals: THEIA_HIP_ERR_INVALID_ARGUMENT before the device is touched, outputs untouched, summary zeroed

def _refused(n, edges, rel, options=None):
    out = np.full((n, 3), 7.0)
    rc, got, est, summ = global_pose.linear_rotations(n, edges, rel, options, orientations_out=out)
    assert rc == capi.THEIA_HIP_ERR_INVALID_ARGUMENT, rc
    assert got is out and np.all(out == 7.0) and not est.any()
    assert (summ.iterations, summ.num_views_in_system) == (0, 0)
    assert list(summ.eigenvalues) == [0.0, 0.0, 0.0]
    assert (summ.subspace_change, summ.shift, summ.setup_ms, summ.factor_ms, summ.iterate_ms) == (0.0,) * 5
    return capi.lib().theia_hip_last_error().decode()


def _tiny():
    s = ls.graph("tiny1")
    return s["n"], s["edges"].copy(), s["rel"].copy()


def test_refuses_no_edge():
    n, e, r = _tiny()
    assert "no relative rotation" in _refused(n, e[:0], r[:0])


def test_refuses_an_edge_out_of_range():
    n, e, r = _tiny()
    e[2, 1] = 4
    assert "out of range" in _refused(n, e, r)
    n, e, r = _tiny()
    e[0, 0] = -1
    assert "out of range" in _refused(n, e, r)


def test_refuses_an_edge_from_a_view_to_itself():
    n, e, r = _tiny()
    e[3] = (2, 2)
    assert "itself" in _refused(n, e, r)


def test_refuses_a_graph_that_is_not_connected():
    n, e, r = _tiny()
    e = np.concatenate([e, [[4, 5]]]).astype(np.int32)
    r = np.concatenate([r, [[0.0, 0.1, 0.0]]])
    assert not ls.connected(6, e)
    assert "not connected" in _refused(6, e, r)


@pytest.mark.parametrize("iters", [0, -3])
def test_refuses_non_positive_max_num_iterations(iters):
    o = global_pose.LinearRotationEstimatorOptions()
    o.max_num_iterations = iters
    assert "max_num_iterations" in _refused(*_tiny(), o)


@pytest.mark.parametrize("thr", [0.0, -1e-10, float("inf"), float("nan")])
def test_refuses_a_bad_threshold(thr):
    o = global_pose.LinearRotationEstimatorOptions()
    o.subspace_convergence_threshold = thr
    assert "subspace_convergence_threshold" in _refused(*_tiny(), o)


def test_defaults_enum_and_exports():
    o = global_pose.LinearRotationEstimatorOptions()
    assert (o.max_num_iterations, o.subspace_convergence_threshold) == (1000, 1e-10)
    c = o.to_c()
    assert (c.max_num_iterations, c.reserved, c.subspace_convergence_threshold) == (1000, 0, 1e-10)
    assert global_pose.GlobalRotationEstimatorType.LINEAR == 2 and sfm.GlobalRotationEstimatorType.LINEAR == 2
    assert sfm.LinearRotationEstimator is global_pose.LinearRotationEstimator
    assert sfm.LinearRotationEstimatorOptions is global_pose.LinearRotationEstimatorOptions
    import ctypes
    assert ctypes.sizeof(capi.LinearRotationOptions) == 16 and ctypes.sizeof(capi.LinearRotationSummary) == 2 * 4 + 8 * 8
    with pytest.raises(ValueError):
        global_pose.linear_rotations(3, [[0, 1], [1, 2]], np.zeros((1, 3)))
    with pytest.raises(ValueError):
        global_pose.linear_rotations(3, [[0, 1]], np.zeros((1, 3)), orientations_out=np.zeros((2, 3)))


# ---- the Python class, with the array call replaced by a recorder (no device)

def _recorder(monkeypatch, rc=0):
    calls = []

    def fake(num_views, edges, relative_rotations, options=None, orientations_out=None):
        calls.append(dict(n=num_views, edges=np.array(edges), rel=np.array(relative_rotations)))
        out = 100.0 + np.arange(3.0 * num_views).reshape(num_views, 3)   # row k = 100 + (3k, 3k + 1, 3k + 2)
        return rc, out, np.ones(num_views, dtype=bool), capi.LinearRotationSummary()

    monkeypatch.setattr(global_pose, "linear_rotations", fake)
    return calls


def _info(x):
    return types.SimpleNamespace(rotation_2=np.array([x, 0.0, 0.0]))


def test_class_indexes_views_by_first_appearance(monkeypatch):
    calls = _recorder(monkeypatch)
    est = sfm.LinearRotationEstimator()
    out = est.EstimateRotations({(70, 13): _info(0.1), (13, 5): _info(0.2), (5, 70): _info(0.3)})
    assert calls[0]["n"] == 3 and calls[0]["edges"].tolist() == [[0, 1], [1, 2], [2, 0]]   # 70 -> 0, 13 -> 1, 5 -> 2
    assert calls[0]["rel"][:, 0].tolist() == [0.1, 0.2, 0.3]
    assert list(out) == [70, 13, 5]
    assert np.array_equal(out[13], [103.0, 104.0, 105.0]) and np.array_equal(out[5], [106.0, 107.0, 108.0])
    assert est.last_success is True and isinstance(est.last_summary, capi.LinearRotationSummary)


def test_class_accumulates_constraints_over_calls(monkeypatch):
    calls = _recorder(monkeypatch)
    est = sfm.LinearRotationEstimator()
    est.AddRelativeRotationConstraint((9, 4), [0.0, 0.5, 0.0])
    est.EstimateRotations({(4, 2): _info(0.1)})
    assert calls[0]["edges"].tolist() == [[0, 1], [1, 2]]            # 9, 4, 2
    out = est.EstimateRotations({(2, 30): _info(0.2)})
    assert calls[1]["n"] == 4 and calls[1]["edges"].tolist() == [[0, 1], [1, 2], [2, 3]]
    assert calls[1]["rel"].tolist() == [[0.0, 0.5, 0.0], [0.1, 0.0, 0.0], [0.2, 0.0, 0.0]]
    assert list(out) == [9, 4, 2, 30]


def test_class_keeps_passed_orientations(monkeypatch):
    _recorder(monkeypatch)
    est = sfm.LinearRotationEstimator()
    given = {13: np.array([1.0, 2.0, 3.0]), 99: np.array([4.0, 5.0, 6.0])}   # 99 is in no pair
    out = est.EstimateRotations({(70, 13): _info(0.1), (13, 5): _info(0.2)}, given)
    assert sorted(out) == [5, 13, 70, 99]
    assert np.array_equal(out[13], [1.0, 2.0, 3.0])                  # emplace does not overwrite
    assert np.array_equal(out[99], [4.0, 5.0, 6.0])
    assert np.array_equal(out[70], [100.0, 101.0, 102.0]) and np.array_equal(out[5], [106.0, 107.0, 108.0])
    assert sorted(given) == [13, 99]                                 # the caller's dict is not modified
    out[13][0] = -1.0
    assert given[13][0] == 1.0


def test_class_reports_failure_and_refusals(monkeypatch):
    with pytest.raises(capi.TheiaHipError) as ex:
        sfm.LinearRotationEstimator().EstimateRotations({})
    assert ex.value.code == capi.THEIA_HIP_ERR_INVALID_ARGUMENT
    _recorder(monkeypatch, rc=capi.THEIA_HIP_ERR_INTERNAL)
    est = sfm.LinearRotationEstimator()
    out = est.EstimateRotations({(1, 2): _info(0.1)})
    assert est.last_success is False and sorted(out) == [1, 2]       # the dict comes back whether the solve succeeded or not
