"""GPU: every LM loop of the library stops where its oracle stops -- by each of the three tolerance rules (at the two values of
a bracket placed on the oracle, tests/lm_rule_cases.py), at the iteration caps, and whatever the number of LM bodies the main
solve enqueues per host synchronisation."""
import numpy as np
import pytest

from pytheiasfm_amd import _capi as capi, ba
from tests import lm_rule_cases as L
from tests import oracle_lib as ol

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ the device side of every case
def _offsets(arrays):
    return np.concatenate([[0], np.cumsum([len(a) for a in arrays])]).astype(np.int64)


def _main(case, ps, o):
    p = ps[0].copy()
    s, tr = ba.solve(p, o)
    return [L.result_of(s, tr, (p.cam_ext, p.points, p.intrinsics))]


def _invdepth(case, ps, o):
    p = ps[0].copy()
    s, tr = ba.solve(p, o)
    return [L.result_of(s, tr, (p.cam_ext, p.point_inverse_depth, p.intrinsics))]


def _views(case, ps, o):
    cams = np.array([p["cam"] for p in ps])
    summ = ba.solve_views_batch(_offsets([p["uv"] for p in ps]), np.vstack([p["uv"] for p in ps]), np.vstack([p["points"] for p in ps]), cams,
                                np.array([p["intr"] for p in ps]), np.array([p["model"] for p in ps], np.int32), o)
    return [L.result_of(summ[k], None, (cams[k],)) for k in range(len(ps))]


def _tracks(case, ps, o):
    pg = case.flat().copy()
    summ = ba.solve_tracks_batch(pg, o)
    return [L.result_of(summ[q], None, (pg.points[q],)) for q in ps]


def _angular(case, ps, o):
    pose = np.array([p["x0"] for p in ps])
    summ = ba.solve_two_views_angular_batch(_offsets([p["corr"] for p in ps]), np.vstack([p["corr"] for p in ps]), pose, o, case.kw["solver"])
    return [L.result_of(summ[k], None, (pose[k],)) for k in range(len(ps))]


def _homography(case, ps, o):
    H = np.array([p["x0"] for p in ps])
    summ = ba.optimize_homography_batch(_offsets([p["corr"] for p in ps]), np.vstack([p["corr"] for p in ps]), H, o)
    return [L.result_of(summ[k], None, (H[k],)) for k in range(len(ps))]


def _fundamental(case, ps, o):
    F = np.array([p["x0"] for p in ps])
    summ = ba.optimize_fundamental_matrix_batch(_offsets([p["corr"] for p in ps]), np.vstack([p["corr"] for p in ps]), F, o)
    return [L.result_of(summ[k], None, (F[k],)) for k in range(len(ps))]


def _two_view_ba(case, ps, o):
    off = _offsets([p["corr"] for p in ps])
    cam_ext = np.array([p["cam_ext"] for p in ps]); intr = np.array([p["intr"] for p in ps]); pts = np.vstack([p["points"] for p in ps])
    summ = ba.solve_two_views_batch(off, np.vstack([p["corr"] for p in ps]), cam_ext, intr, np.zeros((len(ps), 2), np.int32),
                                    np.array([p["const"] for p in ps], np.uint8), pts, o)
    return [L.result_of(summ[k], None, (cam_ext[k, 1], intr[k, :, 0], pts[off[k]:off[k + 1]])) for k in range(len(ps))]


DEVICE = {L.MainCase: _main, L.InvDepthCase: _invdepth, L.ViewsCase: _views, L.TracksCase: _tracks, L.AngularCase: _angular,
          L.HomographyCase: _homography, L.FundamentalCase: _fundamental, L.TwoViewBaCase: _two_view_ba}

# (initial cost, final cost) relative and the parameters, as the neighbouring parity tests of each loop compare them:
# absolute per array unless marked relative to the largest entry ("rel"); tolerances_of() has the main solve's exceptions
COST_TOL = {L.MainCase: (1e-12, 1e-9), L.InvDepthCase: (1e-12, 1e-9), L.ViewsCase: (1e-10, 1e-9), L.TracksCase: (1e-10, 1e-9),
            L.AngularCase: (1e-9, 1e-9), L.HomographyCase: (1e-9, 1e-8), L.FundamentalCase: (1e-9, 1e-7), L.TwoViewBaCase: (1e-12, 1e-8)}
PARAM_TOL = {L.MainCase: (1e-8, 1e-8, ("rel", 1e-9)), L.InvDepthCase: (1e-8, 1e-8, ("rel", 1e-9)), L.ViewsCase: (1e-9,), L.TracksCase: (1e-9,),
             L.AngularCase: (1e-9,), L.HomographyCase: (("rel", 1e-8),), L.FundamentalCase: (("rel", 1e-8),),
             L.TwoViewBaCase: (1e-7, ("rel", 1e-8), ("rel", 1e-6))}


def tolerances_of(case):
    """((initial cost, final cost, trace cost), parameters) of one case.  Costs of the main solve with free intrinsics or priors
    follow test_intrinsics_group_constant_and_bounds / test_camera_priors_match_oracle (1e-8), everything else
    test_lm_trajectory_matches_oracle_c1 (1e-9).  The parameters are held to 1e-8 (intrinsics 1e-9 relative) in every main-solve
    case: these runs stop after a few accepted steps, well inside what the parity tests allow after full convergence, and a
    rejected candidate handed back in place of the last accepted step would be off by a whole step."""
    ti, tf = COST_TOL[type(case)]
    if isinstance(case, L.MainCase) and (case.kw.get("intrinsics_to_optimize") or case.kw.get("priors")):
        return (ti, 1e-8, 1e-8), PARAM_TOL[type(case)]
    return (ti, tf, 1e-9), PARAM_TOL[type(case)]


def device(case, rule, **kw):
    return DEVICE[type(case)](case, case.problems(rule), case.opt(default=ba.default_options, **kw))


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


def _rel_all(a, b):
    return float(np.max(np.abs(a - b) / np.abs(b))) if len(a) else 0.0


def compare(case, r, e, tag):
    """One problem's device result r against its oracle result e; returns the largest parameter difference relative to its bound."""
    worst = 0.0
    assert (r.termination_type, r.num_iterations, r.num_successful_steps, r.success) == \
           (e.termination_type, e.num_iterations, e.num_successful_steps, e.success), (tag, r[:6], e[:6])
    (ti, tf, _), ptol = tolerances_of(case)
    # (+ 1e-20: test_two_views_angular_batch_follows_oracle's floor for costs of normalised coordinates that converge to ~1e-14)
    assert _rel(r.initial_cost, e.initial_cost) <= ti and abs(r.final_cost - e.final_cost) <= tf * abs(e.final_cost) + 1e-20, (tag, r[:6], e[:6])
    for a, b, tol in zip(r.params, e.params, ptol):
        if a.size == 0:
            continue
        d = np.abs(a - b).max()
        bound = tol[1] * np.abs(b).max() if isinstance(tol, tuple) else tol
        assert d <= bound, (tag, d, bound)
        worst = max(worst, d / bound)
    return worst


def compare_trace(case, r, e, rule, tag):
    tr, tro = r.trace, e.trace
    tc = tolerances_of(case)[0][2]
    assert tr.size == tro.size == e.num_iterations + 1, (tag, tr.size, tro.size)
    assert np.array_equal(tr.accepted, tro.accepted), (tag, tr.accepted, tro.accepted)
    # whole trace, in the measure of test_lm_trajectory_matches_oracle_c1 (relative to the largest entry)
    big = lambda a, b: np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)
    assert big(tr.cost, tro.cost) <= tc and big(tr.step_norm, tro.step_norm) <= 1e-6, tag
    # the radius follows rho = cost change / model cost change: compared where the cost change stands 1e9 clear of the rounding of
    # the cost sums (1e-15 relative); below that both sides still accept, but rho is no longer the same number
    clear = np.concatenate([[True], np.abs(np.diff(tro.cost)) >= 1e-6 * tro.cost[:-1]])
    assert _rel_all(tr.radius[clear], tro.radius[clear]) <= 1e-9, tag
    # the last entry: a parameter- or function-tolerance stop records the candidate's cost and step, not accepted.  At the deciding
    # iteration (stop_at, quadratic phase) the step is compared on its own; one iteration later it is built from a gradient that
    # has fallen by another factor of 100 and carries the rounding of x in its last digits (measured: 1.6e-6 relative at 6e-8)
    assert _rel(tr.cost[-1], tro.cost[-1]) <= tc, tag
    if rule in ("function", "parameter"):
        assert tr.accepted[-1] == 0 and tro.accepted[-1] == 0, tag
        if e.num_iterations == case.stop_at[rule]:
            assert _rel(tr.step_norm[-1], tro.step_norm[-1]) <= 1e-6, tag
    elif rule == "gradient":
        assert tr.accepted[-1] == 1, tag


# ------------------------------------------------------------------ the three rules
@pytest.mark.parametrize("case,rule", L.CASE_RULES, ids=lambda v: v if isinstance(v, str) else repr(v))
def test_device_stops_where_the_oracle_stops(case, rule):
    worst = 0.0
    for side in (0, 1):
        v, exp, skip = case.expected(rule, side)
        got = device(case, rule, **L.tolerances(rule, v))
        assert len(got) == len(exp) and len(skip) <= 1
        assert exp[0].termination_type == L.TERM_CONVERGENCE
        assert (exp[0].num_iterations == case.stop_at[rule]) == (side == 0)
        for k, (r, e) in enumerate(zip(got, exp)):
            if k in skip:
                continue
            worst = max(worst, compare(case, r, e, (case, rule, side, k)))
            if e.trace is not None and r.trace is not None:
                compare_trace(case, r, e, rule, (case, rule, side, k))
    print(f"\n[lm-rule parameters] {case.name}-{rule}: largest parameter difference = {worst:.2e} of its bound")


@pytest.mark.parametrize("case", L.TRACED_CASES, ids=repr)
def test_gradient_margin(case):
    """The relative difference between the device's and the oracle's value of each rule's quantity (gradient max norm, step norm,
    |cost change| / cost) at the deciding iteration, printed; the half-width of every bracket is at least 100 times it
    (lm_rule_cases.GRADIENT_MARGINS records the gradient figures)."""
    free = dict(function_tolerance=0.0, gradient_tolerance=0.0, parameter_tolerance=0.0)
    stops = {rule: k for rule, k in case.stop_at.items() if k is not None}
    cap = max(stops.values()) + 1
    r = device(case, "parameter", max_num_iterations=cap, **free)[0]
    e = case.oracle("parameter", case.opt(max_num_iterations=cap, **free))[0]
    assert np.array_equal(r.trace.accepted, e.trace.accepted)
    ratio = lambda t, k: abs(t.cost[k - 1] - t.cost[k]) / t.cost[k - 1]
    quantity = {"gradient": lambda t, k: t.gradient_max_norm[k], "parameter": lambda t, k: t.step_norm[k], "function": ratio}
    diff = {rule: _rel(quantity[rule](r.trace, k), quantity[rule](e.trace, k)) for rule, k in stops.items()}
    print(f"\n[lm-rule margin] {case.name}: " + "  ".join(f"{rule} {d:.3e} (w {case.w[rule]:g})" for rule, d in diff.items()))
    for rule, d in diff.items():
        assert 100.0 * d <= case.w[rule], (case, rule, d)


BATCH_GRADIENT_CASES = [c for c in L.BATCH_CASES if c.stop_at["gradient"] is not None]


@pytest.mark.parametrize("case", BATCH_GRADIENT_CASES, ids=repr)
def test_batched_gradient_margin(case):
    """The batched loops record no trace, so the device's value of the gradient at the deciding iteration is measured through the
    rule itself: the device's own critical gradient tolerance of problem 0, bisected inside the bracket, relative to the oracle's
    t*.  Both are bisected to 1e-6, the resolution of the printed figure; the half-width is at least 100 times it."""
    t, (hi, lo) = case.critical("gradient")
    stop_at = case.stop_at["gradient"]
    early = lambda v: device(case, "gradient", **L.tolerances("gradient", v))[0].num_iterations <= stop_at
    assert early(hi) and not early(lo)
    while hi / lo > 1.0 + 1e-6:
        mid = np.sqrt(hi * lo)
        if early(mid):
            hi = mid
        else:
            lo = mid
    d = abs(np.sqrt(hi * lo) / t - 1.0)
    print(f"\n[lm-rule margin] {case.name}: gradient {d:.3e} (w {case.w['gradient']:g}), through the device's critical tolerance")
    assert 100.0 * d <= case.w["gradient"], (case, d)


# ------------------------------------------------------------------ the iteration caps
CAP_CASES = [L.MAIN_CASES[0], L.INVDEPTH_CASES[0], L.BATCH_CASES[0], [c for c in L.BATCH_CASES if c.name == "angular-cgnr"][0]]


@pytest.mark.parametrize("cap", [0, 1, 2])
@pytest.mark.parametrize("case", CAP_CASES, ids=repr)
def test_iteration_caps_match_oracle(case, cap):
    """max_num_iterations 0, 1, 2 with no tolerance that could end the run: NO_CONVERGENCE at the cap, final_cost = the smallest
    cost seen (+ the fixed cost).  With a gradient tolerance that iteration 0 already satisfies: CONVERGENCE after 0 iterations --
    except at cap 0, where Ceres (and the oracle) look at the iteration count first."""
    free = dict(function_tolerance=0.0, gradient_tolerance=0.0, parameter_tolerance=0.0)
    got = device(case, "gradient", max_num_iterations=cap, **free)
    exp = case.oracle("gradient", case.opt(max_num_iterations=cap, **free))
    for k, (r, e) in enumerate(zip(got, exp)):
        assert (e.termination_type, e.num_iterations) == (L.TERM_NO_CONVERGENCE, cap), (case, cap, k, e[:6])
        compare(case, r, e, (case, cap, k))
        if e.trace is not None and r.trace is not None:
            assert r.trace.size == e.trace.size == cap + 1 and np.array_equal(r.trace.accepted, e.trace.accepted)
        if cap == 0:
            assert r.final_cost == r.initial_cost
            for a, p0 in zip(r.params, device_start(case, k)):
                assert np.array_equal(a, p0), (case, k)             # nothing moved
    big = dict(free, gradient_tolerance=1e30)
    got = device(case, "gradient", max_num_iterations=cap, **big)
    exp = case.oracle("gradient", case.opt(max_num_iterations=cap, **big))
    for k, (r, e) in enumerate(zip(got, exp)):
        want = (L.TERM_NO_CONVERGENCE if cap == 0 else L.TERM_CONVERGENCE, 0, 0)
        assert (e.termination_type, e.num_iterations, e.num_successful_steps) == want, (case, cap, k, e[:6])
        compare(case, r, e, (case, cap, k, "gradient tolerance 1e30"))
        assert r.final_cost == r.initial_cost


def device_start(case, k):
    """The parameters problem k of the case starts from, in the layout of Result.params."""
    p = case.problems("gradient")[k]
    if isinstance(case, L.MainCase):
        return (p.cam_ext, p.points, p.intrinsics)
    if isinstance(case, L.InvDepthCase):
        return (p.cam_ext, p.point_inverse_depth, p.intrinsics)
    if isinstance(case, L.ViewsCase):
        return (p["cam"],)
    return (p["x0"],)


# ------------------------------------------------------------------ LM bodies per host synchronisation
CHUNK_CASES = [c for c in L.MAIN_CASES if c.name in ("main-plain", "main-inner")]


def _same_bits(a, b, tag):
    assert (a.termination_type, a.num_iterations, a.num_successful_steps, a.success) == \
           (b.termination_type, b.num_iterations, b.num_successful_steps, b.success), (tag, a[:6], b[:6])
    assert a.initial_cost == b.initial_cost and a.final_cost == b.final_cost, tag
    assert a.trace.size == b.trace.size, tag
    for name in ("cost", "gradient_max_norm", "step_norm", "radius", "accepted"):
        assert np.array_equal(getattr(a.trace, name), getattr(b.trace, name)), (tag, name)
    for x, y in zip(a.params, b.params):
        assert np.array_equal(x, y), tag


@pytest.mark.parametrize("stop", [2, 3, 4])
@pytest.mark.parametrize("cap", [6, 9])
@pytest.mark.parametrize("case", CHUNK_CASES, ids=repr)
def test_bodies_after_termination_leave_the_state_alone(case, cap, stop, monkeypatch):
    """The main solve enqueues several LM bodies per host synchronisation (one chunk of 6 at cap 6; 4, 4, 1 at cap 9;
    THEIA_HIP_LM_CHUNK overrides) and relies on the bodies after termination being no-ops.  A parameter-tolerance stop at
    iteration 2, 3 or 4 falls on the first, a middle or the last body of a chunk depending on the setting; chunk 1 never runs a
    trailing body.  Summary, trace and parameters are equal to the bit across the settings.  THEIA_HIP_PHASE_TIMING=1 takes the
    unfused control kernel and another tile reduction: same stops, agreement with the oracle to the usual tolerances."""
    t, pair = case.critical("parameter", stop)
    assert t is not None
    kw = dict(L.tolerances("parameter", pair[0]), max_num_iterations=cap)
    e = case.oracle("parameter", case.opt(**kw))[0]
    assert (e.termination_type, e.num_iterations) == (L.TERM_CONVERGENCE, stop)
    runs = {}
    for chunk in (None, "1", "3"):
        if chunk is None:
            monkeypatch.delenv("THEIA_HIP_LM_CHUNK", raising=False)
        else:
            monkeypatch.setenv("THEIA_HIP_LM_CHUNK", chunk)
        runs[chunk] = device(case, "parameter", **kw)[0]
    monkeypatch.delenv("THEIA_HIP_LM_CHUNK", raising=False)
    compare(case, runs["1"], e, (case, cap, stop, "chunk 1"))
    compare_trace(case, runs["1"], e, "parameter", (case, cap, stop, "chunk 1"))
    _same_bits(runs[None], runs["1"], (case, cap, stop, "default chunk vs 1"))
    _same_bits(runs["3"], runs["1"], (case, cap, stop, "chunk 3 vs 1"))
    monkeypatch.setenv("THEIA_HIP_PHASE_TIMING", "1")
    r = device(case, "parameter", **kw)[0]
    monkeypatch.delenv("THEIA_HIP_PHASE_TIMING")
    compare(case, r, e, (case, cap, stop, "phase timing"))
    compare_trace(case, r, e, "parameter", (case, cap, stop, "phase timing"))

