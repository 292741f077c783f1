"""GPU: theia_hip_nonlinear_positions (csrc/nonlinear_positions.hip) against the torch restatement
(tests/nonlinear_position_ref.py), which differentiates the residual by reverse-mode autodiff and solves the full dense
normal equations, points included, on the host.  tests/test_nonlinear_positions.py checks on the CPU that every scene
here gives the restatement decision margins above 1e-3 and reaches the branch it is there for.

Bounds.  The decisions (iterations, the three step counts, the termination, the accepted column of the trace) are equal.
Every other bound is 100 times the restatement's own Cholesky-against-LU difference of the same quantity on the same
scene, computed here.  Short runs from a start near the truth compare positions, points and the trace's costs; the long
runs (a random start, the coincident views, the all-scales scene with its free translation) compare the final cost and
the gauge-invariant (x_j - x_i) / |x_j - x_i| over the edges -- x_j - x_i where every edge carries a scale.  Where the two
host solves agree to within a rounding or two the difference says nothing about another summation order, so each bound
has a floor from the number format alone: 100 roundings of the largest coordinate (100 eps max |x|) for positions and
points; for a relative cost difference the forward bound of a sum of 3 E squares taken in another order, 3 E eps, plus
that of one rounding in each of the two unit vectors a residual is the difference of, 2 eps sqrt(6 E / cost) by
Cauchy-Schwarz over the 3 E components; and 100 eps for a unit direction.  Measured differences: DESIGN.md 3.6l."""
import numpy as np
import pytest

from pytheiasfm_amd import _capi as capi
from pytheiasfm_amd import global_pose, ransac, sfm
from tests import nonlinear_position_ref as ref
from tests import nonlinear_position_scenes as ps

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float64).eps)
ARRAY_KW = ("fixed", "points", "track_offsets", "obs_view", "obs_feature", "ray_orientations", "point_to_camera_weight")


def device(name, **kw):
    s = ps.scene(name)
    kw = {**s["kw"], **kw}
    o = global_pose.NonlinearPositionEstimatorOptions()
    for k, v in kw.items():
        if k not in ARRAY_KW:
            setattr(o, k, v)
    rc, x, pts, summ, trace = global_pose.nonlinear_positions(
        s["aa"], s["init"], s["edges"], s["rel"], s["scales"], options=o, want_trace=True,
        **{k: v for k, v in kw.items() if k in ARRAY_KW})
    assert rc == 0, capi.lib().theia_hip_last_error()
    return x, pts, summ, trace


def same_decisions(summ, trace, o):
    assert (summ.iterations, summ.num_successful_steps, summ.num_unsuccessful_steps, summ.num_invalid_steps,
            summ.termination) == (o["iterations"], o["successful"], o["unsuccessful"], o["invalid"], o["term"])
    assert trace.shape == (len(o["trace"]), 5)
    assert np.array_equal(trace[:, 4], np.array([t[4] for t in o["trace"]], dtype=np.float64))


def _costs(o):
    return np.array([t[0] for t in o["trace"]])


def _cost_floor(name, cost):
    E = _num_edges(name)
    return (3.0 * E + 2.0 * np.sqrt(6.0 * E / cost)) * EPS


def _num_edges(name):
    s = ps.scene(name)
    return len(s["edges"]) + (len(s["kw"]["obs_view"]) if "obs_view" in s["kw"] else 0)


def compare_short(name, got, o, lu):
    """positions, points and trace costs within 100 x the restatement's Cholesky-against-LU spread (module docstring)"""
    x, pts, summ, trace = got
    same_decisions(summ, trace, o)
    full, full_lu, mine = (np.concatenate([a, b]) for a, b in ((o["x"], o["points"]), (lu["x"], lu["points"]), (x, pts)))
    b_x = max(100.0 * np.abs(full - full_lu).max(), 100.0 * EPS * np.abs(full).max())
    b_c = max(100.0 * (np.abs(_costs(o) - _costs(lu)) / _costs(o)).max(), _cost_floor(name, _costs(o).min()))
    d_x = np.abs(mine - full).max()
    d_c = (np.abs(trace[:, 0] - _costs(o)) / _costs(o)).max()
    print("%s: order %d, %d iterations; positions and points %.3g (bound %.3g), trace costs %.3g (bound %.3g)"
          % (name, o["order"], o["iterations"], d_x, b_x, d_c, b_c))
    assert d_x <= b_x and d_c <= b_c
    assert summ.initial_cost == trace[0, 0] and summ.final_cost == trace[trace[:, 4] == 1][-1, 0]
    assert summ.final_radius == trace[-1, 3]


def _edge_quantity(name, x, pts):
    s = ps.scene(name)
    e = s["edges"]
    full = np.concatenate([x, pts])
    if "obs_view" in s["kw"]:
        track = np.repeat(np.arange(len(pts)), np.diff(s["kw"]["track_offsets"]))
        e = np.concatenate([e, np.column_stack([s["kw"]["obs_view"], len(x) + track])])
    d = full[e[:, 1]] - full[e[:, 0]]
    every_edge_scaled = s["scales"] is not None and bool(np.all(s["scales"] > 0.0)) and "obs_view" not in s["kw"]
    return (d, 100.0 * EPS * np.abs(d).max()) if every_edge_scaled else (d / np.linalg.norm(d, axis=1, keepdims=True), 100.0 * EPS)


def compare_long(name, got, o, lu):
    """the decisions, the final cost and the gauge-invariant edge quantity (module docstring)"""
    x, pts, summ, trace = got
    same_decisions(summ, trace, o)
    q, floor = _edge_quantity(name, o["x"], o["points"])
    b_q = max(100.0 * np.abs(q - _edge_quantity(name, lu["x"], lu["points"])[0]).max(), floor)
    b_c = max(100.0 * abs(o["cost"] - lu["cost"]) / o["cost"], _cost_floor(name, o["cost"]))
    d_q = np.abs(_edge_quantity(name, x, pts)[0] - q).max()
    d_c = abs(summ.final_cost - o["cost"]) / o["cost"]
    print("%s: order %d, %d iterations (%d rejected); final cost %.3g (bound %.3g), edge quantity %.3g (bound %.3g)"
          % (name, o["order"], o["iterations"], o["unsuccessful"], d_c, b_c, d_q, b_q))
    assert d_c <= b_c and d_q <= b_q


SHORT = [n for n, (_, want) in ps.CASES.items() if not want.get("long") and n not in ("all_held", "no_edge")]
LONG = [n for n, (_, want) in ps.CASES.items() if want.get("long")]


@pytest.mark.parametrize("name", SHORT)
def test_short_scene(name):
    o, lu = ps.reference(name), ps.reference(name, linear="lu")
    assert o["margin"] > 1e-3
    got = device(name)
    compare_short(name, got, o, lu)
    s, summ = ps.scene(name), got[2]
    held = s["kw"].get("fixed")
    live = int(sum(1 for a, b in s["edges"] if held is None or not (held[a] and held[b])))
    assert 3 * (summ.num_views_in_problem + summ.num_points_in_problem) == o["order"]
    assert (summ.num_camera_edges_in_problem, summ.num_point_edges_in_problem) == (live, _num_edges(name) - len(s["edges"]))
    if held is not None:
        assert np.array_equal(got[0][held], s["init"][held])                 # the bits of a held view
    # determinism: a second call, byte-equal outputs, trace and non-timing summary fields
    again = device(name)
    assert np.array_equal(again[0], got[0]) and np.array_equal(again[1], got[1]) and np.array_equal(again[3], got[3])
    a, b = again[2].as_dict(), summ.as_dict()
    a.pop("seconds"); b.pop("seconds")
    assert a == b


@pytest.mark.parametrize("name", LONG)
def test_long_scene(name):
    o, lu = ps.reference(name), ps.reference(name, linear="lu")
    assert o["margin"] > 1e-3 and lu["iterations"] == o["iterations"]
    got = device(name)
    compare_long(name, got, o, lu)
    again = device(name)
    assert np.array_equal(again[0], got[0]) and np.array_equal(again[3], got[3])


def test_view_without_an_edge_is_untouched():
    o, lu = ps.reference("no_edge"), ps.reference("no_edge", linear="lu")
    got = device("no_edge")
    compare_short("no_edge", got, o, lu)
    assert got[2].num_views_in_problem == 4 and np.array_equal(got[0][4], [7.0, 7.0, 7.0])


def test_every_view_held_is_termination_none():
    s = ps.scene("all_held")
    x, pts, summ, trace = device("all_held")
    assert summ.termination == capi.ROTATION_TERM_NONE and summ.iterations == 0 and trace.shape == (0, 5)
    assert np.array_equal(x, s["init"]) and summ.num_views_in_problem == 0 and summ.num_camera_edges_in_problem == 0


@pytest.mark.parametrize("kind", ps.STOPPING_KINDS)
def test_stopping_rule(kind):
    name, kw, term, iterations = ps.stopping_case(kind)
    o, lu = ps.reference(name, **kw), ps.reference(name, linear="lu", **kw)
    assert o["term"] == term and o["iterations"] == iterations and o["margin"] > 1e-3
    got = device(name, **kw)
    if ps.CASES[name][1].get("long"):
        compare_long(name, got, o, lu)
    else:
        compare_short(name, got, o, lu)
    if kind == "cap0":
        assert np.array_equal(got[0], ps.scene(name)["init"])
    if kind == "gradient":
        assert abs(got[2].final_gradient_max_norm - o["gmaxs"][-1]) <= 1e-9 * o["gmaxs"][-1]
    if kind == "parameter1":
        assert np.array_equal(got[0], ps.scene(name)["init"])             # the step that stops is not taken


def test_refusals_leave_everything_untouched_and_the_device_working():
    s = ps.scene("pts5")
    kw = s["kw"]
    twice = kw["obs_view"].copy(); twice[1] = twice[0]
    nan3 = s["rel"].copy(); nan3[0, 0] = np.nan
    for change in (dict(obs_view=twice), dict(relative_translations=nan3), dict(point_to_camera_weight=-1.0)):
        args = dict(orientations=s["aa"], positions=s["init"], edges=s["edges"], relative_translations=s["rel"], **kw)
        args.update(change)
        rc, x, pts, summ = global_pose.nonlinear_positions(**args)
        assert rc == capi.THEIA_HIP_ERR_INVALID_ARGUMENT and np.array_equal(x, s["init"]) and np.array_equal(pts, kw["points"])
        assert bytes(summ) == bytes(capi.NonlinearPositionSummary())
    x, pts, summ, trace = device("pts5")
    assert summ.iterations == ps.reference("pts5")["iterations"]


def test_mirror_from_view_pairs_to_positions(monkeypatch):
    r, feats, pairs, orientations, s = ps.mirror_case()
    seen = {}
    real = global_pose.nonlinear_positions

    def spy(*a, **kw):
        seen["args"] = (a, kw)
        return real(*a, **kw)

    monkeypatch.setattr(global_pose, "nonlinear_positions", spy)
    est = sfm.NonlinearPositionEstimator(sfm.NonlinearPositionEstimatorOptions(), r, normalized_features=feats)
    est.options.min_num_points_per_view = 2
    est._rng = ransac.RandomNumberGenerator(3)               # the seed tests/test_nonlinear_positions.py checks the margins at
    out = est.EstimatePositions(pairs, orientations)
    a, kw = seen["args"]
    opts = kw.pop("options")
    o = ref.solve(*a, **kw)
    assert o["margin"] > 1e-3 and est.last_success is True and sorted(out) == list(range(5))
    summ = est.last_summary
    assert (summ.iterations, summ.num_successful_steps, summ.num_unsuccessful_steps, summ.num_invalid_steps,
            summ.termination) == (o["iterations"], o["successful"], o["unsuccessful"], o["invalid"], o["term"])
    assert opts is est.options and summ.num_points_in_problem == len(kw["points"]) >= 2
    lu = ref.solve(*a, linear="lu", **kw)
    got = np.array([out[v] for v in range(5)])
    unit = lambda x: (x[s["edges"][:, 1]] - x[s["edges"][:, 0]]) / np.linalg.norm(x[s["edges"][:, 1]] - x[s["edges"][:, 0]], axis=1, keepdims=True)
    b_q = max(100.0 * np.abs(unit(o["x"]) - unit(lu["x"])).max(), 100.0 * EPS)
    d_q = np.abs(unit(got) - unit(o["x"])).max()
    print("mirror: %d iterations; pair directions %.3g (bound %.3g)" % (o["iterations"], d_q, b_q))
    assert d_q <= b_q
    err = np.abs((got[s["edges"][:, 1]] - got[s["edges"][:, 0]]) - (s["gt"][s["edges"][:, 1]] - s["gt"][s["edges"][:, 0]])).max()
    assert err < 0.1                                         # as in tests/test_nonlinear_positions.py
