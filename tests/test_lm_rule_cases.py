"""CPU, oracle only: every case of tests/lm_rule_cases.py has a clean bracket for each of the three tolerance rules, and the
oracle's three rules agree with the third restatement of the loop (tests/independent_lm.py)."""
import numpy as np
import pytest

from tests import independent_lm
from tests import lm_rule_cases as L


def _check_stop(case, rule, r):
    """A CONVERGENCE stop by `rule` of a run without rejected steps: the successful-step count the rule implies."""
    assert r.termination_type == L.TERM_CONVERGENCE and r.success == 1, (case, rule, r[:6])
    want = r.num_iterations if rule == "gradient" else r.num_iterations - 1
    assert r.num_successful_steps == want, (case, rule, r[:6])


@pytest.mark.parametrize("case,rule", L.CASE_RULES, ids=lambda v: v if isinstance(v, str) else repr(v))
def test_bracket_flips_the_oracle(case, rule):
    stop_at = case.stop_at[rule]
    t, pair = case.critical(rule)
    assert t is not None and pair[1] < t < pair[0]
    assert case.w[rule] <= 1e-3
    v_hi, hi, skip_hi = case.expected(rule, 0)
    v_lo, lo, skip_lo = case.expected(rule, 1)
    assert (v_hi, v_lo) == pair
    assert hi[0].num_iterations == stop_at, (case, rule, hi[0][:6])
    assert lo[0].num_iterations > stop_at, (case, rule, lo[0][:6])
    _check_stop(case, rule, hi[0]); _check_stop(case, rule, lo[0])
    assert all(r.success == 1 for r in hi + lo)      # (the other problems of a batch: whatever their own oracle run says)
    assert skip_hi == skip_lo and len(skip_hi) <= 1, (case, rule, skip_hi)
    # quadratic phase: the rule's quantity falls by ten or more to the next iteration
    assert case.fall(rule) >= 10.0, (case, rule, case.fall(rule))
    if rule == "gradient":
        # the stop after stop_at needs one more ACCEPTED step: its cost change must stand clear of the rounding of the cost sums
        if case.free_run(rule).trace is not None:
            t_f = case.cost_change_ratio(rule)[stop_at + 1]
        else:
            run0 = lambda **kw: case.oracle(rule, case.opt(**kw), only=0)[0].num_iterations
            t_f, _ = L.critical_tolerance(run0, "function", stop_at + 1)
        assert t_f is not None and t_f >= 1e-11, (case, t_f)
    if rule == "function":
        assert t >= 1e-3, (case, t)           # |cost change| / cost: a 1e-9 cost difference moves it by <= 1e-6 relative
    if not case.batch:
        # not the noise floor: every step up to the deciding one was accepted in the run without tolerances
        fr = case.free_run(rule)
        assert fr.trace.accepted[: stop_at + (1 if rule == "gradient" else 0)].all() and fr.trace.size > stop_at + 1


def test_batches_stop_at_different_iterations():
    """The point of eight problems per launch: under one bracket value the lanes stop at different iterations."""
    for case in L.BATCH_CASES:
        spread = set()
        for rule in L.RULES:
            if case.stop_at[rule] is None:
                continue
            _, res, _ = case.expected(rule, 0)
            spread |= {r.num_iterations for r in res}
        assert len(spread) >= 2, (case, spread)


@pytest.mark.parametrize("rule", L.RULES)
@pytest.mark.parametrize("case", L.INDEPENDENT_CASES, ids=repr)
def test_independent_lm_stops_where_the_oracle_stops(case, rule):
    """tests/independent_lm.py shares no code with the oracle: at the two bracket values it stops at the same two iterations."""
    o = case.opt()
    for side in (0, 1):
        v, res, _ = case.expected(rule, side)
        free = {0: None, 0x11: [0, 5, 6]}[o.intrinsics_to_optimize]      # FOCAL_LENGTH | RADIAL_DISTORTION of the pinhole model
        trace, cam, pts, intrinsics = independent_lm.solve(
            case.problems(rule)[0].copy(), max_num_iterations=o.max_num_iterations, manifold=bool(o.use_homogeneous_point_parametrization),
            free_intr=free, **L.tolerances(rule, v))
        # iterations = trace entries after the initial one (no invalid steps on these scenes)
        assert len(trace) - 1 == res[0].num_iterations, (case, rule, side, len(trace) - 1, res[0].num_iterations)
        assert [e[4] for e in trace] == list(res[0].trace.accepted)
        assert np.abs(cam - res[0].params[0]).max() <= 1e-7
