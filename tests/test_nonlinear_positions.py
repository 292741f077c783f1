"""CPU: the NONLINEAR position stage without a device -- the torch restatement (tests/nonlinear_position_ref.py) against
central differences and on both sides of the Huber knee, the conditions the GPU scenes must meet (every decision margin
above 1e-3, the branch each scene is there for), the host mirror (track selection, weight, random start against
std::mt19937's documented outputs, the gauge over two calls, skipped pairs) with the restatement in the device's place,
the ABI structures against the header, and the refusals of theia_hip_nonlinear_positions that return before the device
is touched."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from pytheiasfm_amd import _capi as capi
from pytheiasfm_amd import global_pose, ransac, sfm
from pytheiasfm_amd.twoview import TwoViewInfo
from tests import nonlinear_position_ref as ref
from tests import nonlinear_position_scenes as ps
from tests.independent_lm import loss

# ---- the restatement


def _central(f, x, h):
    J = np.zeros((3, 3))
    for k in range(3):
        e = np.zeros(3); e[k] = h
        J[:, k] = (f(x + e) - f(x - e)) / (2.0 * h)
    return J


@pytest.mark.parametrize("branch", ["scaled", "normalised", "tiny"])
def test_restatement_jacobians_against_central_differences(branch):
    rng = np.random.default_rng(11)
    t, w = rng.normal(size=3), 0.7
    xa = rng.normal(size=3)
    xb = xa + rng.normal(size=3)
    if branch == "tiny":                                  # at the origin with a zero direction: every difference is exact
        xa, xb, t = np.zeros(3), np.array([3e-13, -2e-13, 1e-13]), np.zeros(3)
    s = 1.3 if branch == "scaled" else -1.0
    T = lambda v: torch.tensor(np.asarray(v, dtype=np.float64))
    f = lambda a, b: ref.residual(T(a), T(b), T(t), T(w), T(s)).numpy()
    ja, jb = (j.numpy() for j in torch.func.jacrev(ref.residual, argnums=(0, 1))(T(xa), T(xb), T(t), T(w), T(s)))
    h = 1e-6 if branch != "tiny" else 1e-14               # inside the 1e-12 ball the residual is linear in x
    na, nb = _central(lambda v: f(v, xb), xa, h), _central(lambda v: f(xa, v), xb, h)
    # central differences of a smooth function: error ~ h^2 |f'''| + eps |f| / h ~ 1e-10 at h = 1e-6, O(1) values
    tol = 1e-8
    assert np.abs(ja - na).max() < tol and np.abs(jb - nb).max() < tol
    assert np.array_equal(ja, -jb)
    if branch != "normalised":
        assert np.array_equal(jb, w * np.eye(3))
    else:
        d = xb - xa
        u = d / np.linalg.norm(d)
        assert np.abs(jb - w * (np.eye(3) - np.outer(u, u)) / np.linalg.norm(d)).max() < 1e-14


def test_huber_corrector_on_both_sides_of_the_knee():
    a = 0.1
    b = a * a
    s = np.array([0.5 * b, b * (1.0 - 1e-12), b, b * (1.0 + 1e-12), 4.0 * b])
    rho, rho1 = loss("huber", a, s)
    assert np.array_equal(rho[:3], s[:3]) and np.array_equal(rho1[:3], np.ones(3))            # s <= b: the identity
    assert np.allclose(rho[3:], 2.0 * a * np.sqrt(s[3:]) - b, rtol=0, atol=1e-18)
    assert np.allclose(rho1[3:], a / np.sqrt(s[3:]), rtol=1e-15) and abs(rho[4] - 3.0 * b) < 1e-16
    assert abs(rho[3] - rho[2]) < 2e-12 * b and abs(rho1[3] - 1.0) < 1e-12                    # continuous across the knee
    # the restatement scales residual and Jacobian by sqrt(rho'): one scaled edge of length 2 a beyond its target
    P = ref.Problem(np.zeros((2, 3)), [[0, 1]], [[1.0, 0.0, 0.0]], [1.0], None, None, None, None, None, None, 0.5, a)
    x = np.array([[0.0, 0.0, 0.0], [1.0 + 2.0 * a, 0.0, 0.0]])
    cost, r, J = P.evaluate(x, True)
    k = np.sqrt(a / (2.0 * a))
    assert abs(cost - 0.5 * (2.0 * a * 2.0 * a - b)) < 1e-16 and np.allclose(r, [2.0 * a * k, 0.0, 0.0], atol=1e-16)
    assert np.allclose(J, k * np.hstack([-np.eye(3), np.eye(3)]), atol=1e-16)


# ---- the conditions on the GPU scenes


@pytest.mark.parametrize("name", list(ps.CASES))
def test_scene_meets_its_conditions(name):
    want = ps.CASES[name][1]
    o = ps.reference(name)
    assert o["order"] == want["order"]
    if name == "all_held":
        assert o["term"] == ref.TERM_NONE and o["iterations"] == 0
        return
    lu = ps.reference(name, linear="lu")
    assert o["margin"] > 1e-3 and lu["margin"] > 1e-3
    assert (lu["iterations"], lu["successful"], lu["unsuccessful"], lu["term"]) == (
        o["iterations"], o["successful"], o["unsuccessful"], o["term"])
    assert all(o["seen"][k] for k in want["seen"]), o["seen"]
    assert o["invalid"] == 0 and o["term"] == ref.TERM_FUNCTION and o["cost"] < o["initial_cost"]
    if want.get("rejected"):
        assert o["unsuccessful"] >= 1
    if want.get("long"):
        assert o["iterations"] >= 10
    else:
        assert o["iterations"] <= 5 and o["unsuccessful"] == 0
    if name == "tiny3":                                  # the branch at iteration 0 only: the first step separates the two
        assert np.array_equal(ps.scene(name)["init"][0], ps.scene(name)["init"][1]) and o["trace"][1][4] == 1
    if name == "held30":
        s = ps.scene(name)
        assert np.array_equal(o["x"][s["kw"]["fixed"]], s["init"][s["kw"]["fixed"]])
        assert any(s["kw"]["fixed"][a] and s["kw"]["fixed"][b] for a, b in s["edges"])


@pytest.mark.parametrize("kind", ps.STOPPING_KINDS)
def test_stopping_case_meets_its_conditions(kind):
    name, kw, term, iterations = ps.stopping_case(kind)
    o = ps.reference(name, **kw)
    assert o["term"] == term and o["iterations"] == iterations and o["margin"] > 1e-3
    if kind == "parameter2":                             # the stale |x| would decide the same way only within the margin
        base = ps.reference(name, function_tolerance=0.0)
        assert abs(base["x_norms"][1] - base["x_norms"][0]) / base["x_norms"][0] > 1e-3


# ---- the host mirror, the restatement in the device's place

MT19937_5489 = [3499211612, 581869302, 3890346734, 3586334585, 545404204, 4161255391]    # std::mt19937's first outputs


def _rand_double(lo32, hi32, a, b):
    """std::uniform_real_distribution<double>(a, b) on two 32-bit draws (libstdc++'s generate_canonical)."""
    return (float(lo32) + float(hi32) * 4294967296.0) / 18446744073709551616.0 * (b - a) + a


def _options(**kw):
    o = sfm.NonlinearPositionEstimatorOptions()
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_exports_structures_and_constructor_checks():
    assert sfm.NonlinearPositionEstimator is global_pose.NonlinearPositionEstimator
    assert sfm.NonlinearPositionEstimatorOptions is global_pose.NonlinearPositionEstimatorOptions
    assert global_pose.GlobalPositionEstimatorType.NONLINEAR == 0
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "theia_hip.h")).read()
    for struct, cls in (("theia_nonlinear_position_options", capi.NonlinearPositionOptions),
                        ("theia_nonlinear_position_summary", capi.NonlinearPositionSummary)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                kind, names = decl.split(None, 1)
                fields += [(n.strip(), {"int32_t": ctypes.c_int32, "double": ctypes.c_double}[kind]) for n in names.split(",")]
        assert fields == list(cls._fields_)
    assert ctypes.sizeof(capi.NonlinearPositionOptions) == 2 * 4 + 5 * 8
    assert ctypes.sizeof(capi.NonlinearPositionSummary) == 10 * 4 + 5 * 8
    o = _options().to_c()
    assert (o.max_num_iterations, o.robust_loss_width, o.function_tolerance, o.gradient_tolerance, o.parameter_tolerance,
            o.max_trust_region_radius) == (400, 0.1, 1e-6, 1e-10, 1e-8, 1e16)
    d = _options()
    assert (d.rng, d.num_threads, d.min_num_points_per_view, d.point_to_camera_weight) == (None, 1, 0, 0.5)
    for bad in (dict(num_threads=0), dict(min_num_points_per_view=-1), dict(point_to_camera_weight=0.0),
                dict(robust_loss_width=0.0)):
        with pytest.raises(capi.TheiaHipError) as ex:
            sfm.NonlinearPositionEstimator(_options(**bad), sfm.Reconstruction())
        assert ex.value.code == capi.THEIA_HIP_ERR_INVALID_ARGUMENT


def _hand_made():
    """6 views, 6 tracks.  Track: views.  0: 0 1 2 3;  1: 0 1;  2: 0 1 2;  3: 3 4;  4: 3 4 5;  5: 4 (view 5 has one feature)."""
    r = sfm.Reconstruction()
    sees = {0: [0, 1, 2, 3], 1: [0, 1], 2: [0, 1, 2], 3: [3, 4], 4: [3, 4, 5], 5: [4]}
    r.cam_ext = np.zeros((6, 6)); r.cam_ext[:, 3:6] = 0.01 * np.arange(18).reshape(6, 3)
    r.view_estimated = np.ones(6, dtype=bool)
    r.points = np.column_stack([np.arange(18.0).reshape(6, 3) + 1.0, np.full(6, 2.0)])
    r.track_estimated = np.array([True, True, False, True, True, True])
    r.obs_track = np.array([t for t in sees for _ in sees[t]], dtype=np.int32)
    r.obs_view = np.array([v for t in sees for v in sees[t]], dtype=np.int32)
    r.obs_uv = 0.01 * np.arange(2 * len(r.obs_view)).reshape(-1, 2)
    return r


def test_track_selection_and_weight(monkeypatch):
    r = _hand_made()
    est = sfm.NonlinearPositionEstimator(_options(min_num_points_per_view=2, rng=ransac.RandomNumberGenerator(7)), r,
                                         normalized_features=r.obs_uv)
    positions = {v: np.zeros(3) for v in (0, 1, 2, 3, 4)}                    # view 5 has no position
    chosen, count = est._find_tracks(positions)
    # view 0: tracks by (-views, id) = 0 (4 views), 2 (3), 1 (2): takes 0 and 2 -> views 0, 1, 2 have two, view 3 one;
    # views 1, 2: already at two; view 3: unused tracks 4 (3 views), 3 (2): takes 4 -> view 3 two, view 4 one (view 5
    # has no position); view 4: unused 3, 5: takes 3 -> view 4 two, view 3 three
    assert list(chosen) == [0, 2, 4, 3] and chosen == {0: True, 2: False, 4: True, 3: True}
    assert count == 2 + 2 + 2 + 3 + 2
    # through EstimateRemainingPositionsInRecon: the weight, the points' start, the un-estimated track without edges
    monkeypatch.setattr(global_pose, "nonlinear_positions", ps.restatement_as_device)
    r.cam_ext[:, :3] = np.random.default_rng(1).normal(0.0, 3.0, (6, 3))
    pairs = {}
    for a, b in ((0, 1), (1, 2), (2, 3), (3, 4), (0, 4), (4, 5), (2, 9)):     # (4, 5), (2, 9): a view outside the sub-reconstruction
        pairs[(a, b)] = TwoViewInfo()
        pairs[(a, b)].position_2 = np.array([0.6, 0.0, 0.8])
    pairs[(1, 2)].scale_estimate = 2.5
    before = ransac.RandomNumberGenerator(7).get_state()
    ok, out = est.EstimateRemainingPositionsInRecon({0}, {0, 1, 2, 3, 4}, pairs)
    got = ps.restatement_as_device.args
    assert ok is True and sorted(out) == [0, 1, 2, 3, 4] and np.array_equal(out[0], r.cam_ext[0, :3])
    assert np.array_equal(got["edges"], [[0, 1], [1, 2], [2, 3], [3, 4], [0, 4]])              # the two stray pairs skipped
    assert np.array_equal(got["scales"], [-1.0, 2.5, -1.0, -1.0, -1.0])
    assert np.array_equal(got["fixed"], [True, False, False, False, False])
    assert got["weight"] == 0.5 * 5.0 / 11.0
    assert np.array_equal(got["points"], r.points[[0, 3, 4], :3] / 2.0)                        # track 2 is un-estimated
    assert np.array_equal(got["track_offsets"], [0, 4, 6, 8]) and list(got["obs_view"]) == [0, 1, 2, 3, 3, 4, 3, 4]
    assert np.array_equal(got["ray_orientations"], r.cam_ext[:5, 3:6])                         # the views' stored orientations
    assert np.array_equal(got["obs_feature"], r.obs_uv[[0, 1, 2, 3, 9, 10, 11, 12]])
    # the fixed set was given: no random start; the un-estimated track 2 drew its three numbers
    rng = ransac.RandomNumberGenerator(7)
    rng.set_state(before)
    want = 100.0 * np.array([rng.RandDouble(-1.0, 1.0) for _ in range(3)])
    assert sorted(est.triangulated_points) == [0, 2, 3, 4] and np.array_equal(est.triangulated_points[2], want)


def test_random_start_gauge_and_second_call(monkeypatch):
    monkeypatch.setattr(global_pose, "nonlinear_positions", ps.restatement_as_device)
    s = ps.scene("n6_scales")
    ids = [5 + 2 * k for k in range(6)]
    pairs = {}
    for (a, b), t, sc in zip(s["edges"], s["rel"], s["scales"]):
        pairs[(ids[a], ids[b])] = TwoViewInfo()
        pairs[(ids[a], ids[b])].position_2, pairs[(ids[a], ids[b])].scale_estimate = np.array(t), float(sc)
    stray = TwoViewInfo(); stray.position_2 = np.array([1.0, 0.0, 0.0])
    pairs[(5, 1000)] = stray                                                   # view 1000 has no orientation: no position
    orientations = {ids[k]: s["aa"][k] for k in range(6)}
    orientations[99] = np.zeros(3)                                             # no pair names view 99: no position
    rng = ransac.RandomNumberGenerator(5489)
    est = sfm.NonlinearPositionEstimator(_options(rng=rng, max_num_iterations=0), sfm.Reconstruction())
    out = est.EstimatePositions(pairs, orientations)
    want = 100.0 * np.array([_rand_double(MT19937_5489[2 * k], MT19937_5489[2 * k + 1], -1.0, 1.0) for k in range(3)])
    start = ps.restatement_as_device.args["positions"]
    assert np.array_equal(start[0], np.zeros(3))             # the smallest id drew `want` first, then became the origin
    after = rng.get_state()                                  # every generator object is a view of the thread's one
    follow = ransac.RandomNumberGenerator(5489)
    drawn = 100.0 * np.array([follow.RandDouble(-1.0, 1.0) for _ in range(18)]).reshape(6, 3)
    assert np.array_equal(drawn[0], want) and np.array_equal(start[1:], drawn[1:])             # increasing id, x y z
    assert after[2] == follow.get_state()[2] and np.array_equal(after[1], follow.get_state()[1])
    assert sorted(out) == ids and est.last_success is True
    assert ps.restatement_as_device.args["fixed"] is None and len(ps.restatement_as_device.args["edges"]) == 10
    assert ps.restatement_as_device.args["points"] is None
    # the second call: view 5 is recorded as fixed, EstimatePositions starts from no positions: FindOrDie
    with pytest.raises(capi.TheiaHipError) as ex:
        est.EstimatePositions(pairs, orientations)
    assert ex.value.code == capi.THEIA_HIP_ERR_INVALID_ARGUMENT
    # SetViewsFixed and the sub-reconstruction route hold the views and draw nothing
    r = sfm.Reconstruction()
    r.cam_ext = np.zeros((16, 6)); r.cam_ext[ids, :3] = s["init"]; r.cam_ext[ids, 3:6] = s["aa"]
    est = sfm.NonlinearPositionEstimator(_options(rng=rng), r)
    at = rng.get_state()
    ok, out = est.EstimateRemainingPositionsInRecon([7, 9], set(ids), pairs)
    assert ok and np.array_equal(ps.restatement_as_device.args["fixed"], [False, True, True, False, False, False])
    assert np.array_equal(out[7], s["init"][1]) and np.array_equal(out[9], s["init"][2]) and rng.get_state()[2] == at[2]
    assert ps.restatement_as_device.last["margin"] > 1e-3
    assert est.EstimatePositions({}, orientations) == {} and est.last_success is False
    assert est.EstimatePositions(pairs, {}) == {} and est.last_success is False


def test_mirror_with_points_recovers_the_scene(monkeypatch):
    monkeypatch.setattr(global_pose, "nonlinear_positions", ps.restatement_as_device)
    r, feats, pairs, orientations, s = ps.mirror_case()
    est = sfm.NonlinearPositionEstimator(_options(min_num_points_per_view=2, rng=ransac.RandomNumberGenerator(3)), r,
                                         normalized_features=feats)
    out = est.EstimatePositions(pairs, orientations)        # from the random start, the solve's orientations given
    o, args = ps.restatement_as_device.last, ps.restatement_as_device.args
    assert est.last_success and o["margin"] > 1e-3 and o["order"] == 3 * (5 + len(args["points"])) and len(args["points"]) >= 2
    assert not np.array_equal(args["ray_orientations"], args["orientations"]) and args["fixed"] is None
    assert np.array_equal(args["ray_orientations"], r.cam_ext[:, 3:6])
    got = np.array([out[v] for v in range(5)])
    err = np.abs((got[s["edges"][:, 1]] - got[s["edges"][:, 0]]) - (s["gt"][s["edges"][:, 1]] - s["gt"][s["edges"][:, 0]])).max()
    print("mirror, restatement as the solver:", o["iterations"], "iterations, baseline error", err)
    # half the pairs carry their true baseline length and every direction 0.3 degrees of noise on baselines of 1 .. 4
    assert err < 0.1


# ---- refusals that return before the device is touched


def test_refusals_leave_everything_untouched():
    s = ps.scene("pts5")
    kw = dict(s["kw"])
    base = dict(orientations=s["aa"], positions=s["init"], edges=s["edges"], relative_translations=s["rel"], **kw)

    def variant(**change):
        v = dict(base); v.update(change)
        return v

    nan3 = s["rel"].copy(); nan3[2, 1] = np.nan
    inf_pos = s["init"].copy(); inf_pos[0, 0] = np.inf
    off_flat = kw["track_offsets"].copy(); off_flat[3] = off_flat[2]
    twice = kw["obs_view"].copy(); twice[1] = twice[0]
    far = kw["obs_view"].copy(); far[0] = 5
    self_edge = s["edges"].copy(); self_edge[1] = [2, 2]
    out_edge = s["edges"].copy(); out_edge[0] = [0, 5]
    bad_feature = kw["obs_feature"].copy(); bad_feature[0, 0] = np.nan
    cases = [variant(edges=None, relative_translations=None, points=None),                      # no edges of either kind
             variant(edges=out_edge), variant(edges=self_edge), variant(relative_translations=nan3),
             variant(positions=inf_pos), variant(track_offsets=off_flat), variant(obs_view=twice), variant(obs_view=far),
             variant(obs_feature=bad_feature), variant(point_to_camera_weight=0.0),
             variant(point_to_camera_weight=float("inf")), variant(scale_estimates=np.full(len(s["edges"]), np.nan))]
    for opts in (dict(robust_loss_width=0.0), dict(robust_loss_width=float("nan")), dict(function_tolerance=-1.0),
                 dict(gradient_tolerance=-1e-3), dict(parameter_tolerance=float("nan")), dict(max_num_iterations=-1),
                 dict(max_trust_region_radius=0.0)):
        cases.append(variant(options=_options(**opts)))
    for c in cases:
        rc, x, pts, summ = global_pose.nonlinear_positions(**c)
        assert rc == capi.THEIA_HIP_ERR_INVALID_ARGUMENT, c
        assert np.array_equal(x, c["positions"], equal_nan=True) and bytes(summ) == bytes(capi.NonlinearPositionSummary())
        if c.get("points") is not None:
            assert np.array_equal(pts, c["points"])
    lib = capi.lib()
    summ = capi.NonlinearPositionSummary()
    x = np.ascontiguousarray(s["init"]); aa = np.ascontiguousarray(s["aa"])
    e = np.ascontiguousarray(s["edges"], dtype=np.int32); t = np.ascontiguousarray(s["rel"])
    P = lambda a, ct: capi.ptr(a, ct)
    # num_points > 0 with a null array; no views
    rc = lib.theia_hip_nonlinear_positions(5, P(aa, ctypes.c_double), P(x, ctypes.c_double), None, len(e), P(e, ctypes.c_int32),
                                           P(t, ctypes.c_double), None, 3, None, None, None, None, None, 0.5, None,
                                           ctypes.byref(summ), None, 0)
    assert rc == capi.THEIA_HIP_ERR_INVALID_ARGUMENT
    rc = lib.theia_hip_nonlinear_positions(0, P(aa, ctypes.c_double), P(x, ctypes.c_double), None, len(e), P(e, ctypes.c_int32),
                                           P(t, ctypes.c_double), None, 0, None, None, None, None, None, 0.5, None,
                                           ctypes.byref(summ), None, 0)
    assert rc == capi.THEIA_HIP_ERR_INVALID_ARGUMENT and np.array_equal(x, s["init"])
    with pytest.raises(ValueError):
        global_pose.nonlinear_positions(s["aa"], s["init"], s["edges"], s["rel"][:3])
    with pytest.raises(ValueError):
        global_pose.nonlinear_positions(s["aa"], s["init"], s["edges"], s["rel"], fixed=[True])
