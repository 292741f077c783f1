"""GPU: theia_hip_nonlinear_rotations (csrc/nonlinear_rotations.hip) against the torch restatement
(tests/nonlinear_rotation_ref.py), which differentiates the residual by reverse-mode autodiff and solves the full dense
normal equations on the host.

Bounds.  Chain-initialised scenes: 1e-8 rad on the orientations (the bound of tests/test_rotation_averaging_gpu.py; the
restatement's own Cholesky / LU / permutation spread is 2e-13) and 1e-10 relative on the trace's costs.  The
rejected-step scene runs 34 iterations from a random start with the gauge free, so only gauge-invariant quantities are
compared, each within 100 times the restatement's own Cholesky-against-LU difference on that scene.  Measured
differences: DESIGN.md 3.6i."""
import numpy as np
import pytest

from pytheiasfm_amd import _capi as capi
from pytheiasfm_amd import global_pose, sfm
from pytheiasfm_amd.twoview import TwoViewInfo
from tests import nonlinear_rotation_ref as ref
from tests import rotation_scenes as rs
from tests.rotation_averaging_ref import aa_to_R

pytestmark = pytest.mark.gpu

CHAIN_SCENES = {
    "n4_noise1": (4, 6, 1.0, 0.0, 1),
    "n21": (21, 80, 2.0, 0.0, 1),
    "n22_outliers": (22, 80, 2.0, 0.1, 2),
    "n43_outliers": (43, 300, 2.0, 0.1, 3),
    "n100_outliers": (100, 800, 2.0, 0.1, 1),
    "n60_duplicates": (60, 500, 2.0, 0.1, 1),
    "n300_outliers": (300, 3000, 2.0, 0.1, 1),
}
_scenes, _refs = {}, {}


def scene(name):
    if name not in _scenes:
        s = rs.make_scene(*CHAIN_SCENES[name])
        if name == "n60_duplicates":
            s = rs.with_duplicates(s, 25, 25)
        _scenes[name] = s
    return _scenes[name]


def reference(name, **kw):
    key = (name, tuple(sorted((k, v if np.isscalar(v) else tuple(np.asarray(v).tolist())) for k, v in kw.items())))
    if key not in _refs:
        s = scene(name)
        _refs[key] = ref.solve(s["init"], s["edges"], s["rel"], **kw)
    return _refs[key]


def device(s, x0=None, fixed=None, **opts):
    o = global_pose.NonlinearRotationEstimatorOptions()
    for k, v in opts.items():
        setattr(o, k, v)
    rc, out, summ, trace = global_pose.nonlinear_rotations(s["init"] if x0 is None else x0, s["edges"], s["rel"], fixed, o,
                                                           want_trace=True)
    assert rc == 0, capi.lib().theia_hip_last_error()
    return out, summ, trace


def same_decisions(summ, o):
    assert (summ.iterations, summ.num_successful_steps, summ.num_unsuccessful_steps, summ.num_invalid_steps,
            summ.termination) == (o["iterations"], o["successful"], o["unsuccessful"], o["invalid"], o["term"])


def trace_costs_close(trace, o, rel):
    want = np.array([t[0] for t in o["trace"]])
    assert trace.shape == (len(want), 5)
    assert np.array_equal(trace[:, 4], np.array([t[4] for t in o["trace"]], dtype=np.float64))
    d = np.abs(trace[:, 0] - want) / want
    print("trace cost difference (relative, max):", d.max())
    assert d.max() <= rel


@pytest.mark.parametrize("name", list(CHAIN_SCENES))
def test_chain_initialised_scene(name):
    s, o = scene(name), reference(name)
    assert o["margin"] > 1e-3
    out, summ, trace = device(s)
    same_decisions(summ, o)
    diff = rs.angle_between(out, o["x"]).max()
    print(name, "order", 3 * summ.num_views_in_problem, "orientation difference (rad, max):", diff)
    assert diff <= 1e-8
    trace_costs_close(trace, o, 1e-10)
    assert summ.initial_cost == trace[0, 0] and summ.final_cost == trace[trace[:, 4] == 1][-1, 0]
    assert summ.final_radius == trace[-1, 3]
    again, summ2, trace2 = device(s)
    assert np.array_equal(again, out) and np.array_equal(trace2, trace) and summ2.final_cost == summ.final_cost
    assert rs.aligned_errors_deg(out, s["gt"]).max() < rs.aligned_errors_deg(s["init"], s["gt"]).max()


def test_noise_free_scene_takes_no_iteration():
    s = rs.make_scene(4, 6, 0.0, 0.0, 1)
    out, summ, trace = device(s)
    assert summ.iterations == 0 and summ.termination == capi.ROTATION_TERM_GRADIENT_TOLERANCE
    assert np.array_equal(out, s["init"]) and trace.shape == (1, 5) and summ.final_cost < 1e-28


def _relative_rotations(x, edges):
    R = aa_to_R(x)
    return R[edges[:, 1]] @ np.transpose(R[edges[:, 0]], (0, 2, 1))


def test_rejected_step_scene_gauge_invariants():
    s = rs.make_scene(10, 25, 5.0, 0.4, seed=19)
    x0 = np.random.default_rng(119).uniform(-2.5, 2.5, (10, 3))
    kw = dict(robust_loss_width=0.01)
    o = ref.solve(x0, s["edges"], s["rel"], **kw)
    lu = ref.solve(x0, s["edges"], s["rel"], linear="lu", **kw)
    assert o["margin"] > 1e-3 and o["unsuccessful"] == 7 and lu["iterations"] == o["iterations"]
    out, summ, trace = device(s, x0=x0, **kw)
    same_decisions(summ, o)
    # bounds: 100 x the restatement's own Cholesky-against-LU difference on this scene
    c_ref, c_lu = np.array([t[0] for t in o["trace"]]), np.array([t[0] for t in lu["trace"]])
    b_cost = 100.0 * abs(o["cost"] - lu["cost"]) / o["cost"]
    b_rel = 100.0 * np.abs(_relative_rotations(o["x"], s["edges"]) - _relative_rotations(lu["x"], s["edges"])).max()
    b_trace = 100.0 * (np.abs(c_ref - c_lu) / c_ref).max()
    d_cost = abs(summ.final_cost - o["cost"]) / o["cost"]
    d_rel = np.abs(_relative_rotations(out, s["edges"]) - _relative_rotations(o["x"], s["edges"])).max()
    d_trace = (np.abs(trace[:, 0] - c_ref) / c_ref).max()
    print("rejected-step scene: final cost %.3g (bound %.3g), R_j R_i' %.3g (bound %.3g), trace costs %.3g (bound %.3g)"
          % (d_cost, b_cost, d_rel, b_rel, d_trace, b_trace))
    assert np.array_equal(trace[:, 4], np.array([t[4] for t in o["trace"]], dtype=np.float64))
    assert d_cost <= b_cost and d_rel <= b_rel and d_trace <= b_trace


@pytest.mark.parametrize("cap", [0, 1, 2])
def test_iteration_cap(cap):
    s, o = scene("n21"), reference("n21", max_num_iterations=cap)
    assert o["term"] == ref.TERM_CAP and o["iterations"] == cap
    out, summ, trace = device(s, max_num_iterations=cap)
    same_decisions(summ, o)
    assert rs.angle_between(out, o["x"]).max() <= 1e-8
    trace_costs_close(trace, o, 1e-10)
    if cap == 0:
        assert np.array_equal(out, s["init"])


def _between(a, b):
    assert a > 0.0 and b > 0.0 and a != b
    return float(np.sqrt(a * b))


def test_gradient_tolerance_after_the_first_accepted_step():
    s, base = scene("n21"), reference("n21")
    tol = _between(base["gmaxs"][0], base["gmaxs"][1])          # below the start's gradient, above the first step's
    assert base["gmaxs"][1] < tol < base["gmaxs"][0]
    o = reference("n21", gradient_tolerance=tol)
    assert o["term"] == ref.TERM_GRADIENT and o["iterations"] == 1 and o["margin"] > 1e-3
    out, summ, trace = device(s, gradient_tolerance=tol)
    same_decisions(summ, o)
    assert rs.angle_between(out, o["x"]).max() <= 1e-8
    assert abs(summ.final_gradient_max_norm - o["gmaxs"][-1]) <= 1e-9 * o["gmaxs"][-1]


def test_parameter_tolerance_at_iteration_one_reads_the_initial_x_norm():
    s, base = scene("n21"), reference("n21")
    # stop when step_norm <= tol (x_norm + tol): tol between the step's ratio and ten times it
    ratio = base["step_norms"][0] / base["x_norms"][0]
    tol = _between(ratio, 10.0 * ratio)
    o = reference("n21", parameter_tolerance=tol)
    assert o["term"] == ref.TERM_PARAMETER and o["iterations"] == 1 and o["margin"] > 1e-3
    out, summ, trace = device(s, parameter_tolerance=tol)
    same_decisions(summ, o)
    assert np.array_equal(out, s["init"])
    trace_costs_close(trace, o, 1e-10)


def test_parameter_tolerance_at_iteration_two_reads_the_refreshed_x_norm():
    s, base = scene("n21"), reference("n21", function_tolerance=0.0)
    r1, r2 = base["step_norms"][0] / base["x_norms"][0], base["step_norms"][1] / base["x_norms"][1]
    assert r2 < r1
    tol = _between(r1, r2)                                       # the first step passes, the second stops
    o = reference("n21", function_tolerance=0.0, parameter_tolerance=tol)
    assert o["term"] == ref.TERM_PARAMETER and o["iterations"] == 2 and o["margin"] > 1e-3
    # the stale |x| would decide the same way only if it were within the margin: the two norms differ by more
    assert abs(base["x_norms"][1] - base["x_norms"][0]) / base["x_norms"][0] > 1e-3
    out, summ, trace = device(s, function_tolerance=0.0, parameter_tolerance=tol)
    same_decisions(summ, o)
    assert rs.angle_between(out, o["x"]).max() <= 1e-8
    assert abs(trace[-1, 2] - o["trace"][-1][2]) <= 1e-9 * o["trace"][-1][2]


@pytest.mark.parametrize("held", [(17,), (0, 3, 50, 51, 99)])
def test_fixed_views(held):
    s = scene("n100_outliers")
    fixed = np.zeros(100, dtype=bool); fixed[list(held)] = True
    o = reference("n100_outliers", fixed=fixed)
    assert o["margin"] > 1e-3
    out, summ, trace = device(s, fixed=fixed)
    same_decisions(summ, o)
    assert summ.num_views_in_problem == 100 - len(held)
    assert np.array_equal(out[fixed], s["init"][fixed])
    assert rs.angle_between(out, o["x"]).max() <= 1e-8
    trace_costs_close(trace, o, 1e-10)


def test_view_without_an_edge_is_untouched():
    s = scene("n21")
    x0 = np.concatenate([s["init"], [[0.3, -0.2, 0.1]], [[7.0, 7.0, 7.0]]])          # views 21 and 22 have no edge
    o = reference("n21")
    rc, out, summ = global_pose.nonlinear_rotations(x0, s["edges"], s["rel"])
    assert rc == 0 and summ.num_views_in_problem == 21
    assert np.array_equal(out[21:], x0[21:])
    assert rs.angle_between(out[:21], o["x"]).max() <= 1e-8 and summ.iterations == o["iterations"]


def test_near_singular_systems_are_steps_not_errors():
    s = rs.make_scene(8, 20, 2.0, 0.1, 1)
    x0 = np.random.default_rng(7).uniform(-1.5, 1.5, (8, 3))
    out, summ, trace = device(s, x0=x0, function_tolerance=0.0)
    assert np.isfinite(summ.final_cost) and summ.final_cost <= summ.initial_cost
    counted = summ.num_successful_steps + summ.num_unsuccessful_steps + summ.num_invalid_steps
    # a pass that ends on the parameter or function tolerance is in none of the three counts (theia_hip.h)
    ended_in_pass = summ.termination in (capi.ROTATION_TERM_PARAMETER_TOLERANCE, capi.ROTATION_TERM_FUNCTION_TOLERANCE)
    assert counted == summ.iterations - (1 if ended_in_pass else 0)
    assert summ.termination != capi.ROTATION_TERM_NONE and np.all(np.isfinite(out))
    print("near-singular run:", summ.as_dict())


def test_refusals_leave_everything_untouched():
    s = scene("n21")
    before = s["init"].copy()
    for edges, rel, opts in ((np.zeros((0, 2), dtype=np.int32), np.zeros((0, 3)), {}),
                             (np.array([[0, 21]], dtype=np.int32), s["rel"][:1], {}),
                             (np.array([[4, 4]], dtype=np.int32), s["rel"][:1], {}),
                             (s["edges"], s["rel"], dict(robust_loss_width=0.0)),
                             (s["edges"], s["rel"], dict(function_tolerance=float("nan"))),
                             (s["edges"], s["rel"], dict(max_num_iterations=-1))):
        o = global_pose.NonlinearRotationEstimatorOptions()
        for k, v in opts.items():
            setattr(o, k, v)
        rc, out, summ = global_pose.nonlinear_rotations(before, edges, rel, None, o)
        assert rc == capi.THEIA_HIP_ERR_INVALID_ARGUMENT and np.array_equal(out, before)
        assert bytes(summ) == bytes(capi.NonlinearRotationSummary())
    rc, out, summ = global_pose.nonlinear_rotations(before, s["edges"], s["rel"])        # and the device still works after them
    assert rc == 0 and summ.iterations == reference("n21")["iterations"]


def _view_pairs(s, ids):
    pairs = {}
    weights = np.random.default_rng(3).permutation(len(s["edges"])) + 30       # an outlier pair has few matches
    weights[s["outliers"]] -= 25 + np.arange(int(s["outliers"].sum()))
    for (a, b), r, w in zip(s["edges"], s["rel"], weights):
        info = TwoViewInfo()
        info.rotation_2 = np.array(r)
        info.num_verified_matches = int(w)
        pairs[(ids[a], ids[b])] = info
    return pairs


@pytest.mark.parametrize("seed_with", ["spanning_tree", "linear"])
def test_mirror_from_view_pairs_to_refined_orientations(seed_with):
    s = scene("n22_outliers")
    ids = [7 + 3 * k for k in range(22)]                                    # non-contiguous, ascending
    pairs = _view_pairs(s, ids)
    if seed_with == "spanning_tree":
        seed = sfm.OrientationsFromMaximumSpanningTree(pairs)
    else:
        seed = sfm.LinearRotationEstimator().EstimateRotations(pairs)
    assert sorted(seed) == ids
    stray = TwoViewInfo()
    stray.rotation_2 = np.array([0.5, 0.5, 0.5])
    pairs[(7, 1000)] = stray                                               # view 1000 has no orientation: skipped
    keep = {v: np.array(r) for v, r in seed.items()}
    est = sfm.NonlinearRotationEstimator()
    out = est.EstimateRotations(pairs, seed)
    assert est.last_success is True and sorted(out) == ids
    assert all(np.array_equal(seed[v], keep[v]) for v in ids)
    assert est.last_summary.termination == capi.ROTATION_TERM_FUNCTION_TOLERANCE and est.last_summary.iterations > 0
    got = np.array([out[v] for v in ids])
    # the scene's tolerance: the pairs carry 2 degrees of noise each, and a view's error after averaging over its pairs is
    # below that of a single pair unless the solve ends in another basin, where it is tens of degrees: 1.5 x the noise
    err = rs.aligned_errors_deg(got, s["gt"]).max()
    print(seed_with, "aligned error (degrees):", err)
    assert err < 3.0
