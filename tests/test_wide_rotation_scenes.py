"""CPU: the scenes of tests/wide_rotation_scenes.py are fair tests before any GPU sees them -- computed with the
restatements only.  Every scene has a third or more of its orientations in the trace < 0 half of the matrix logarithm and
the seven planted rows; the nonlinear scenes start with each of the four logarithm branches on two edges or more, none of
them a near tie; and every decision the GPU tests compare as an integer (iteration counts, terminations, base pairs,
triangle gates, the filters' verdicts) is far from its threshold in the restatement."""
import numpy as np
import pytest

from tests import filter_scenes as fs
from tests import linear_rotation_ref as lr
from tests import lud_positions_ref
from tests import nonlinear_rotation_ref as nref
from tests import rotation_averaging_ref as rar
from tests import translation_filter_ref as tf
from tests import wide_rotation_scenes as ws

EPS = np.finfo(float).eps


def _negative_trace_share(aa):
    return float((np.trace(rar.aa_to_R(aa), axis1=1, axis2=2) < 0.0).mean())


def _planted(aa):
    return np.array_equal(aa[1:8], ws.PLANTED)


def test_full_sphere_orientations():
    aa = ws.full_sphere_orientations(500, 3)
    angle = np.linalg.norm(aa, axis=1)
    assert _planted(aa) and angle.max() <= np.pi and angle[8:].min() > 0.0
    # angle U(0, pi): a third beyond 2 pi / 3, where the trace is negative; axis from a normal draw: no preferred direction
    assert abs(_negative_trace_share(aa[8:]) - 1.0 / 3.0) < 0.07
    assert np.abs((aa[8:] / angle[8:, None]).mean(0)).max() < 0.1
    assert not _planted(ws.full_sphere_orientations(7, 3)) and ws.full_sphere_orientations(7, 3).shape == (7, 3)
    # the planted rows: three half turns about the axes, one about the diagonal (equal diagonal entries), and both sides of
    # ceres' small-angle branch
    R = rar.aa_to_R(ws.PLANTED)
    assert np.allclose(np.diagonal(R[3]), -1.0 / 3.0) and [int(np.argmax(np.diagonal(R[k]))) for k in range(3)] == [0, 1, 2]
    t2 = (ws.PLANTED * ws.PLANTED).sum(1)
    assert 0.0 < t2[5] < EPS and t2[6] == 0.0 and t2[4] > EPS


@pytest.mark.parametrize("name", list(ws.ROTATION_CASES))
def test_rotation_averaging_scenes(name):
    s, fixed = ws.rotation_case(name)
    assert _planted(s["gt"]) and _negative_trace_share(s["gt"]) >= 1.0 / 3.0 and _negative_trace_share(s["init"]) >= 1.0 / 3.0
    assert np.array_equal(s["edges"][:s["n"] - 1], np.stack([np.arange(s["n"] - 1), np.arange(1, s["n"])], 1))
    assert not s["outliers"][:s["n"] - 1].any()
    r = ws.cached(("rotation_ref", name), lambda: rar.robust_rotation_averaging(s["init"], s["edges"], s["rel"], fixed))
    print(name, "min margin", min(m for _, m in r["margins"]), (r["l1_iterations"], r["admm_iterations"], r["irls_iterations"]))
    assert min(m for _, m in r["margins"]) > 1e-6


def test_planted_outliers_take_the_three_diagonal_branches_in_turn():
    s, _ = ws.rotation_case("w66_outliers")
    branch, margin = ws.residual_branches(s["gt"], s["edges"], s["rel"])
    q = np.arange(int(s["outliers"].sum()))
    assert len(q) == 50 and np.array_equal(branch[s["outliers"]], 1 + q % 3) and margin[s["outliers"]].min() > 1e-6
    assert np.all(branch[~s["outliers"]] == 0)


def _nonlinear_fair(x0, s, o):
    branch, margin = ws.residual_branches(x0, s["edges"], s["rel"])
    count = np.bincount(branch, minlength=4)
    print("branches", count, "smallest branch margin", margin.min(), "decision margin", o["margin"],
          (o["iterations"], o["successful"], o["term"]))
    assert count.min() >= 2
    assert margin.min() > 1e-6
    assert o["margin"] > 1e-3


@pytest.mark.parametrize("name", list(ws.NONLINEAR_CASES))
def test_nonlinear_scenes(name):
    s = ws.nonlinear_case(name)
    assert _planted(s["gt"]) and _negative_trace_share(s["gt"]) >= 1.0 / 3.0 and _negative_trace_share(s["init"]) >= 1.0 / 3.0
    o = ws.cached(("nonlinear_ref", name), lambda: nref.solve(s["init"], s["edges"], s["rel"]))
    _nonlinear_fair(s["init"], s, o)
    assert o["iterations"] >= 2 and o["successful"] >= 2


def test_nonlinear_held_views_scene():
    s = ws.nonlinear_case("w22")
    fixed = np.zeros(s["n"], dtype=bool)
    fixed[ws.HELD] = True
    x0 = ws.noisy_start(s, 2.0, fixed, seed=5)
    assert np.array_equal(x0[fixed], ws.PLANTED)             # held at the exact planted vectors
    o = ws.cached(("nonlinear_ref", "held"), lambda: nref.solve(x0, s["edges"], s["rel"], fixed=fixed))
    _nonlinear_fair(x0, s, o)
    # every planted row has an edge onto a free view: aa_rot runs at pi, at pi - 1e-9 and in the small-angle branch
    live = fixed[s["edges"][:, 0]] != fixed[s["edges"][:, 1]]
    assert set(ws.HELD) <= set(s["edges"][live].ravel())


@pytest.mark.parametrize("name", list(ws.LINEAR_CASES))
def test_linear_rotation_scenes(name):
    s = ws.linear_case(name)
    assert _planted(s["gt"]) and _negative_trace_share(s["gt"]) >= 1.0 / 3.0
    assert float(np.linalg.norm(s["rel"], axis=1).max()) > 3.0          # relative rotations close to pi, not the 40 degrees of rotation_scenes
    r = lr.reference(s["n"], s["edges"], s["rel"])
    d = lr.device_steps(s["n"], s["edges"], s["rel"])
    w = r["eigenvalues"]
    print(name, "reference against device_steps", lr.gauge_free_angles(r["orientations"], d["orientations"]).max(),
          "iterations", d["iterations"], "lambda_3 / lambda_4", w[2] / w[3])
    assert d["converged"] and d["iterations"] <= 19                      # the GPU test allows one more and at most 20
    assert w[2] / w[3] <= 0.2                                            # the contraction test_linear_rotations_gpu.py's bound assumes
    assert lr.gauge_free_angles(r["orientations"], d["orientations"]).max() <= 1e-9


@pytest.mark.parametrize("name", list(ws.LUD_CASES))
def test_lud_scenes(name):
    s = ws.lud_case(name)
    assert _planted(s["orientations"]) and _negative_trace_share(s["orientations"]) >= 1.0 / 3.0
    r = ws.cached(("lud_ref", name), lambda: lud_positions_ref.lud_positions(s["orientations"], s["edges"], s["rel"],
                                                                                np.arange(s["n"]) < 1))
    print(name, "min margin", min(r["margins"]), r["admm_iterations"], r["converged"])
    assert min(r["margins"]) > 1e-6


def _in_front(s):
    """Every observation of an orbit scene has a finite feature of a point in front of its camera: the cameras look at the
    origin from 16 or more away and the points lie within sqrt(3) of it."""
    return bool(np.isfinite(s["obs_feature"]).all() and np.abs(s["obs_feature"]).max() < 0.2)


@pytest.mark.parametrize("name", list(ws.LIGT_CASES))
def test_ligt_orbit_scenes(name):
    s, r = ws.ligt_case(name)
    assert _negative_trace_share(s["orientations"]) >= 1.0 / 3.0 and _in_front(s)
    used = r["base_pairs"][:, 0] >= 0
    assert used.all()
    assert np.all(r["theta_gap"][used] > 1e-9), r["theta_gap"][used].min()      # the tie rule of test_ligt_positions.py
    w = r["eigenvalues"]
    print(name, "theta gap", r["theta_gap"][used].min(), "eigenvalues", w[:2], w[-1], "votes", r["votes"])
    assert abs(w[0]) <= 64 * len(w) * EPS * w[-1] and w[1] > 1e-7 * w[-1]       # one null vector, as test_ligt_positions.py
    assert r["votes"] != 0


def test_a_ligt_orbit_scene_exercises_the_flip():
    assert any(ws.ligt_case(name)[1]["votes"] < 0 for name in ws.LIGT_CASES)


@pytest.mark.parametrize("name", list(ws.TRIPLET_CASES))
def test_triplet_orbit_scenes(name):
    s, r = ws.triplet_case(name)
    assert _negative_trace_share(s["orientations"]) >= 1.0 / 3.0 and _in_front(s)
    assert float(np.linalg.norm(s["rot"], axis=1).max()) > 2.9
    assert r["gate_margin"].min() > 0.0 and r["gate_margin"].min() >= 1e-9
    assert np.all(np.isinf(r["ftv_margin"]) | (r["ftv_margin"] >= 1e-9))
    assert np.all(s["edges"][:, 0] < s["edges"][:, 1]) and np.all(r["state"] == 0)
    w = r["eigenvalues"]
    print(name, "gate margin", r["gate_margin"].min(), "eigenvalues", w[:2], w[-1])
    assert abs(w[0]) <= 64 * len(w) * EPS * w[-1] and w[1] > 1e-7 * w[-1]


def test_orientation_filter_scene():
    s = ws.orientation_filter_case()
    assert _planted(s["orientations"]) and _negative_trace_share(s["orientations"]) >= 1.0 / 3.0
    want, margin = tf.filter_orientations(s["edges"], s["orientations"], s["rel"], ws.FILTER_DEGREES)
    assert abs(s["turned_deg"] / ws.FILTER_DEGREES - 1.0).min() > 1e-6 and margin > 1e-6
    assert np.array_equal(want, s["turned_deg"] > ws.FILTER_DEGREES)
    near = s["turned_deg"] < 2.0 * ws.FILTER_DEGREES
    assert want[near].sum() >= 20 and (~want[near]).sum() >= 20            # both sides of the threshold


def test_translation_filter_scene():
    p = ws.translation_filter_case()
    assert _planted(p["orientations"]) and _negative_trace_share(p["orientations"]) >= 1.0 / 3.0
    r = tf.filter_translations(p["n"], p["pairs"], p["orientations"], p["position_2"], 48, 0.08, 
                               axes=fs.unit_axes(48, seed=ws.TRANSLATION_FILTER_AXES_SEED))
    assert r["min_gap"] >= 1e-9 and r["threshold_margin"] >= 1e-9           # the admission rule of test_view_pair_filters_gpu.py
    assert 0 < r["removed"].sum() < len(r["removed"])
