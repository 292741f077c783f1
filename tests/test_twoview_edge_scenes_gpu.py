"""GPU: the three wavefront LM kernels of csrc/twoview_lm.hip (k_twoview_lm, k_homography_lm, k_fundamental_lm) through
ba.solve_two_views_angular_batch, ba.optimize_homography_batch and ba.optimize_fundamental_matrix_batch on the cases of
tests/twoview_edge_scenes.py: correspondence counts 0 .. 129 around the parameter counts and the wave tails, positions at and
next to the poles of SphereManifold<3>, zero / first-order / near-pi rotations, clamped and valid residuals in one problem,
degenerate H0 and F0, every case at full length (where test_twoview_edge_scenes.py admits it) and as its first step "@1".

  * every case alone against the oracle: counts and termination equal, poses to 1e-9 absolute, H and F to 1e-8 relative, costs
    to 1e-9 / 1e-8 relative (the tolerances of test_two_views_angular_batch_follows_oracle and test_optimize_*_batch_*), and
    what a solve must keep: |position| = 1, H(2, 2) = 1, a failed or empty problem returns its input;
  * in batches of 2, 3, 4, 5 and 9 in two orders, with empty problems first, in the middle and last and a problem that fails
    at iteration 0 in the wave slots 0 and 3: bit-identical to the solo run (the kernels are wave-uniform, the butterfly's
    order is fixed);
  * the first step against tests/twoview_lm_ref.py (autodiff, nothing shared with oracle/ or csrc/) at the bounds that
    test_twoview_edge_scenes.py derived from the oracle; the initial cost against a numpy.longdouble sum;
  * the refusals leave their outputs untouched.

Measured on an MI355X (every case prints its figures): the largest deviation of any case from the oracle, in units of its
tolerance, was 0.18 for a final cost (angular n2 / cgnr / truncated, two correspondences: a cost of 1e-14; the next is
0.014, homography n1 "@1"), 0.013 for a pose (south / cgnr / trivial, 1.3e-11 absolute), 2e-4 for an H (h22zero "@1"), 1e-3 for an
F (fullrank, 12 iterations) and 7e-5 for an initial cost.  The first step lay 1.9e-12 (angular, rot1e-7), 1.1e-12
(homography, h22zero) and 3.4e-13 (fundamental, fullrank) from the independent one, the initial cost 1.9e-12 relative from the
long-double sum: the oracle's own figures.
What these tests found: under the TRUNCATED loss a singular H0 had the finite initial cost n e / 2 and converged at iteration 0
(fmin drops the NaN that std::min(s, e) of loss_functions.cc:40-44 returns), where the oracle and the TRIVIAL loss fail at
iteration 0; the kernels now keep a NaN squared norm (loss_eval_nan).  An empty fundamental problem failed after five invalid
steps; it now converges at iteration 0 like the other two.
Deliberately wrong builds, for the record (arithmetic only, each in a scratch copy, run once, never committed):
  * beta = 2 -> 0 in householder3's sigma <= DBL_EPSILON branch: the 24 pole- and nearpole- cases of
    test_case_follows_the_oracle fail, and test_device_first_step_is_the_independent_step[angular]; nothing else;
  * the sign of the second column of fund_plus_jacobian: 38 fundamental cases (every one that takes a step from a start of
    rank 2 or 3) and the independent step [fundamental];
  * the lane-63 term dropped from wsum: the 230 cases with 64 correspondences or more (lane 63 holds one) and none of the
    others, the independent step and the initial cost of all three kinds;
  * the sign of R(0, 1) in aa_to_rot's first-order branch: the 12 rot5e-9 cases, the independent step and the initial cost
    [angular], and fundamental nearequal at 12 iterations (a step of fund_plus that small); rot0 cannot see it (w = 0)."""
import functools
import itertools

import numpy as np
import pytest

from pytheiasfm_amd import _capi as capi, ba
from tests import twoview_edge_scenes as tes
from tests import twoview_lm_ref as ref

pytestmark = pytest.mark.gpu

PROBLEM = {"angular": ref.Angular, "homography": ref.Homography, "fundamental": ref.Fundamental}
KINDS = ("angular", "homography", "fundamental")


def _summary(s):
    return dict(success=int(s.success), termination_type=int(s.termination_type), num_iterations=int(s.num_iterations),
                num_successful_steps=int(s.num_successful_steps), initial_cost=float(s.initial_cost), final_cost=float(s.final_cost))


def group_of(case):
    """cases of one group can share a launch: the options and the solver are per batch"""
    return (case.kind, case.solver, case.loss, case.width, case.iters)


def device(cases):
    """one launch over the cases (of one group); returns [(result, summary dict)]"""
    first = cases[0]
    assert all(group_of(c) == group_of(first) for c in cases)
    offsets = np.concatenate([[0], np.cumsum([c.n for c in cases])]).astype(np.int64)
    corr = np.vstack([c.corr for c in cases]).reshape(-1, 4)
    x = np.ascontiguousarray(np.array([c.x0 for c in cases], dtype=np.float64))
    o = first.set_options(ba.default_options())
    if first.kind == "angular":
        summ = ba.solve_two_views_angular_batch(offsets, corr, x, o, first.solver)
    elif first.kind == "homography":
        summ = ba.optimize_homography_batch(offsets, corr, x, o)
    else:
        summ = ba.optimize_fundamental_matrix_batch(offsets, corr, x, o)
    return [(x[i].copy(), _summary(summ[i])) for i in range(len(cases))]


@functools.lru_cache(maxsize=None)
def solo(name):
    return device([tes.CASES[name]])[0]


@functools.lru_cache(maxsize=None)
def oracle(name):
    return tes.solve_oracle(tes.CASES[name])


def input_of(case):
    """what a solve that does nothing returns: the homography entry still divides by H(2, 2)"""
    with np.errstate(all="ignore"):
        return case.x0 / case.x0[2, 2] if case.kind == "homography" else case.x0


@pytest.mark.parametrize("name", list(tes.CASES))
def test_case_follows_the_oracle(name):
    case = tes.CASES[name]
    got, want = solo(name), oracle(name)
    same, dev = tes.deviations(case, got, want)
    print(f"DEV {name} x {dev['x']:.3e} c0 {dev['initial_cost']:.3e} c1 {dev['final_cost']:.3e} "
          f"it {got[1]['num_iterations']} ns {got[1]['num_successful_steps']} term {got[1]['termination_type']}")
    assert same, (name, got[1], want[1])
    assert max(dev.values()) <= 1.0, (name, dev)
    x, s = got
    if case.kind == "angular" and s["num_successful_steps"] > 0:
        assert abs(np.linalg.norm(x[3:]) - 1.0) <= 1e-14, (name, np.linalg.norm(x[3:]) - 1.0)
    if case.kind == "homography" and np.all(np.isfinite(x)):
        assert x[2, 2] == 1.0, (name, x[2, 2])
    if s["termination_type"] == tes.FAILURE or case.n == 0:
        assert s["num_successful_steps"] == 0 and np.array_equal(x, input_of(case), equal_nan=True), (name, x)
    if s["num_successful_steps"] == 0:                      # nothing accepted: the same holds
        assert np.array_equal(x, input_of(case), equal_nan=True), (name, x)


# ------------------------------------------------------------------ batch shapes
# E: an empty problem, F: one that fails at iteration 0, o: the next case of the group.  Two orders; sizes 2, 3, 4, 5, 9:
# the empties first, in the middle and last, the failing one in wave slots 0 and 3 (problem p runs on wave p % 4)
TEMPLATES = (("Eo", "oEo", "FooF", "oooFE", "EooFEoooE"), ("oE", "Foo", "FooF", "Eoooo", "FooooEooF"))
GROUPS = {}
for _name, _case in tes.CASES.items():
    GROUPS.setdefault(group_of(_case), []).append(_name)
del _name, _case


def batches_of(names):
    """[(order, [names])]: every case of the group in at least one batch of each order"""
    empties = [n for n in names if tes.CASES[n].n == 0]
    failing = [n for n in names if n.split("/")[1].split("@")[0] in ("singular", "zero")]
    others = [n for n in names if n not in empties and n not in failing]
    out = []
    for order, seq in enumerate((others, others[::-1])):
        feed = itertools.cycle(seq)
        used = 0
        for template in itertools.cycle(TEMPLATES[order]):
            batch = []
            for slot in template:
                pool = empties if slot == "E" else failing if slot == "F" else None
                if pool:
                    batch.append(pool[0])
                else:
                    batch.append(next(feed)); used += 1
            out.append((order, batch))
            if used >= len(seq) and len(out) % len(TEMPLATES[order]) == 0:
                break
    return out


def test_batch_templates():
    for order in TEMPLATES:
        assert [len(t) for t in order] in ([2, 3, 4, 5, 9],)
    text = "".join(TEMPLATES[0] + TEMPLATES[1])
    assert any(t[0] == "E" for t in TEMPLATES[0] + TEMPLATES[1]) and any(t[-1] == "E" for t in TEMPLATES[0] + TEMPLATES[1])
    assert any("E" in t[1:-1] for t in TEMPLATES[0] + TEMPLATES[1]) and "F" in text
    slots = {i % 4 for t in TEMPLATES[0] + TEMPLATES[1] for i, c in enumerate(t) if c == "F"}
    assert {0, 3} <= slots
    # every kind has a group with an empty problem; the homography and fundamental groups have a failing one
    for kind in KINDS:
        assert any(k[0] == kind and any(tes.CASES[n].n == 0 for n in names) for k, names in GROUPS.items())
    for k, names in GROUPS.items():
        if k[0] != "angular":
            assert any(n.split("/")[1].split("@")[0] in ("singular", "zero") for n in names), k


@pytest.mark.parametrize("key", list(GROUPS), ids=lambda k: f"{k[0]}-s{k[1]}-l{k[2]}-i{k[4]}")
def test_batches_are_bit_identical_to_solo_runs(key):
    names = GROUPS[key]
    seen = [set(), set()]
    for order, batch in batches_of(names):
        out = device([tes.CASES[n] for n in batch])
        for slot, (n, (x, s)) in enumerate(zip(batch, out)):
            xs, ss = solo(n)
            assert np.array_equal(x, xs, equal_nan=True), (batch, slot, n)
            for k in ss:
                assert s[k] == ss[k] or (np.isnan(s[k]) and np.isnan(ss[k])), (batch, slot, n, k, s[k], ss[k])
            seen[order].add(n)
    assert seen[0] == set(names) and seen[1] == set(names)


# ------------------------------------------------------------------ the independent first step
@functools.lru_cache(maxsize=None)
def independent(name):
    case = tes.CASES[name]
    return ref.first_step(PROBLEM[case.kind](case.corr, case.loss, case.width), case.x0)


@pytest.mark.parametrize("kind", KINDS)
def test_device_first_step_is_the_independent_step(kind):
    worst = (0.0, "")
    for name, case in tes.CASES.items():
        if not (case.kind == kind and name.endswith("@1") and tes.has_unique_basis(name) and case.solver == tes.EXACT):
            continue
        x, s = solo(name)
        x_ref, _, accepted, iterations = independent(name)
        assert s["num_successful_steps"] == int(accepted) and s["num_iterations"] == iterations, (name, s, accepted, iterations)
        if np.array_equal(x, x_ref, equal_nan=True):
            d = 0.0
        elif kind == "angular":
            d = float(np.abs(x - x_ref).max())
        else:
            d = float(np.abs(x - x_ref).max() / np.abs(x_ref).max())
        worst = max(worst, (d, name))
        assert d <= tes.STEP_BOUND[kind], (name, d)
    print(f"STEP {kind}: largest deviation of the device's first step from the independent one {worst[0]:.3e} ({worst[1]}), "
          f"bound {tes.STEP_BOUND[kind]:.1e}")
    assert worst[1]


@pytest.mark.parametrize("kind", KINDS)
def test_device_initial_cost_is_the_long_double_sum(kind):
    """every "@1" case, CGNR and NO_UNIQUE_BASIS included (the initial cost does not depend on the iteration count)"""
    worst = (0.0, "")
    for name, case in tes.CASES.items():
        if not (case.kind == kind and name.endswith("@1")):
            continue
        got = solo(name)[1]["initial_cost"]
        want = ref.initial_cost_longdouble(PROBLEM[kind](case.corr, case.loss, case.width), case.x0)
        if not np.isfinite(want):
            assert not np.isfinite(got), name
            continue
        d = abs(got - want) / want if want else abs(got)
        worst = max(worst, (d, name))
        assert d <= tes.INITIAL_COST_BOUND, (name, d)
    print(f"COST {kind}: largest relative deviation of the device's initial cost {worst[0]:.3e} ({worst[1]}), bound {tes.INITIAL_COST_BOUND:.1e}")


# ------------------------------------------------------------------ refusals
def _refused(call, *arrays):
    before = [a.copy() for a in arrays]
    with pytest.raises(capi.TheiaHipError):
        call()
    for a, b in zip(arrays, before):
        assert np.array_equal(a, b)


def test_refusals_leave_the_outputs_untouched():
    ang = [tes.CASES["angular/n5/exact/truncated@1"], tes.CASES["angular/n6/exact/truncated@1"]]
    hom = [tes.CASES["homography/n5/truncated@1"], tes.CASES["homography/n63/truncated@1"]]
    fun = [tes.CASES["fundamental/n7@1"], tes.CASES["fundamental/n8@1"]]
    entries = ((ang, lambda off, c, x, o, solver=ba.TWO_VIEW_EXACT: ba.solve_two_views_angular_batch(off, c, x, o, solver)),
               (hom, lambda off, c, x, o: ba.optimize_homography_batch(off, c, x, o)),
               (fun, lambda off, c, x, o: ba.optimize_fundamental_matrix_batch(off, c, x, o)))
    for cases, call in entries:
        corr = np.vstack([c.corr for c in cases])
        n0, n1 = cases[0].n, cases[1].n
        x = np.ascontiguousarray(np.array([c.x0 for c in cases]))
        good = cases[0].set_options(ba.default_options())
        _refused(lambda: call(np.array([0, n0 + n1, n0], dtype=np.int64), corr, x, good), x)              # decreasing offsets
        _refused(lambda: call(np.array([1, n0, n0 + n1], dtype=np.int64), corr, x, good), x)              # offsets[0] != 0
        bad = cases[0].set_options(ba.default_options()); bad.max_num_iterations = -1
        _refused(lambda: call(np.array([0, n0, n0 + n1], dtype=np.int64), corr, x, bad), x)               # negative iterations
    corr = np.vstack([c.corr for c in ang]); x = np.ascontiguousarray(np.array([c.x0 for c in ang]))
    off = np.array([0, ang[0].n, ang[0].n + ang[1].n], dtype=np.int64)
    for solver in (2, -1):
        _refused(lambda: entries[0][1](off, corr, x, ang[0].set_options(ba.default_options()), solver), x)  # an unknown solver
    corr = np.vstack([c.corr for c in fun]); x = np.ascontiguousarray(np.array([c.x0 for c in fun]))
    off = np.array([0, fun[0].n, fun[0].n + fun[1].n], dtype=np.int64)
    for loss in (tes.HUBER, tes.TRUNCATED):
        o = fun[0].set_options(ba.default_options()); o.loss_function_type = loss
        _refused(lambda: entries[2][1](off, corr, x, o), x)                                                # a loss on the F entry
