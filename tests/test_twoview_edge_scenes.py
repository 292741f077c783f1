"""CPU: the oracle alone on the cases of tests/twoview_edge_scenes.py (oracle_two_views_angular, oracle_optimize_homography,
oracle_optimize_fundamental: what tests/test_twoview_edge_scenes_gpu.py compares the kernels of csrc/twoview_lm.hip with).

a. Admission.  The oracle runs every case again with the correspondences in a fixed permuted order, and once more with every
   coordinate one unit in the last place up.  A case is admitted when the iteration count, the successful steps, the
   termination and success agree with both and the results and costs differ by at most a TENTH of the device tolerance
   (twoview_edge_scenes.deviations).  Every "@1" form is admitted, and the full-length cases that are not are exactly the
   literal AT_ONE_ONLY.  The permutation alone admitted seven cases that no arithmetic can reproduce to the tolerance: with
   one or two correspondences a sum does not depend on its order, and neither does it when the TRUNCATED loss leaves one
   or two residuals; their final costs are round-off (1e-13 .. 1e-18, relative deviations up to 3e-5 on the device).
b. Independent step.  The oracle's "@1" result against tests/twoview_lm_ref.first_step (autodiff residuals, manifolds from their
   definitions, the step rules of tests/independent_lm.py) on every case with the exact solver outside NO_UNIQUE_BASIS; the
   CGNR cases (an inexact step by design) and the others compare the initial cost only, which every case compares (at
   max_num_iterations = 0) with a numpy.longdouble sum of the independent residuals.
   Measured here (largest deviation over the cases; the bound is ten times that):
     angular      1.96e-12 absolute (rot1e-7, a rotation just outside aa_to_rot's first-order branch, where 1 - cos(theta) =
                  5e-15 keeps two digits; every other case <= 1.4e-13)     bound 2e-11
     homography   4.96e-13 relative (n1)                                     bound 5e-12
     fundamental  4.25e-13 relative (fullrank)                               bound 4.3e-12
     initial cost 3.15e-12 relative (homography n1: one correspondence)      bound 3.2e-11
   No case needs more than 1e-9.
c. Failure and empty paths: an empty problem is CONVERGENCE at iteration 0 with both costs 0 and its input untouched -- for
   the fundamental matrix too, where the loop would otherwise take five invalid steps (model cost change 0) and FAIL --; the
   singular H0 and the zero F0 are FAILURE at iteration 0 with a non-finite initial cost.
The scenes' conventions are fixed by the independent residuals vanishing on the noise-free data."""
import functools

import numpy as np
import pytest

from tests import twoview_edge_scenes as tes
from tests import twoview_lm_ref as ref

KINDS = ("angular", "homography", "fundamental")
STEP_BOUND, INITIAL_COST_BOUND = tes.STEP_BOUND, tes.INITIAL_COST_BOUND            # shared with the GPU test
PROBLEM = {"angular": ref.Angular, "homography": ref.Homography, "fundamental": ref.Fundamental}


@functools.lru_cache(maxsize=None)
def oracle(name):
    return tes.solve_oracle(tes.CASES[name])


def admitted(case, first):
    for other in (case.permuted(), case.nudged()):
        same, dev = tes.deviations(case, tes.solve_oracle(other), first)
        if not (same and max(dev.values()) <= 0.1):
            return False
    return True


def at_one(kind):
    return [n for n, c in tes.CASES.items() if c.kind == kind and n.endswith("@1")]


@functools.lru_cache(maxsize=None)
def independent(name):
    """(x after the first step, initial cost, accepted, iterations) of the independent reference; shared by the tests that need it"""
    case = tes.CASES[name]
    return ref.first_step(PROBLEM[case.kind](case.corr, case.loss, case.width), case.x0)


def step_deviation(case, x, x_ref):
    """absolute for the pose, relative to the largest entry for H and F; 0 where both are the same bits (NaN included)"""
    if np.array_equal(x, x_ref, equal_nan=True):
        return 0.0
    if case.kind == "angular":
        return float(np.abs(x - x_ref).max())
    return float(np.abs(x - x_ref).max() / np.abs(x_ref).max())


def compares_step(name):
    case = tes.CASES[name]
    return name.endswith("@1") and tes.has_unique_basis(name) and case.solver == tes.EXACT


def test_case_table():
    """the table is complete: the counts, the poses, the starts, every case as "@1", the literals consistent"""
    for n in tes.ANGULAR_COUNTS:
        for solver in ("exact", "cgnr"):
            for loss in (("trivial", "huber", "truncated") if n >= 5 else ("truncated",)):
                assert f"angular/n{n}/{solver}/{loss}@1" in tes.CASES
    assert tes.ANGULAR_COUNTS == (0, 1, 2, 3, 4, 5, 6, 63, 64, 65, 127, 128, 129)
    assert tes.HOMOGRAPHY_COUNTS == (0, 1, 2, 3, 4, 5, 63, 64, 65, 129) and tes.FUNDAMENTAL_COUNTS == (0, 1, 2, 6, 7, 8, 63, 64, 65, 129)
    assert max(c.n for c in tes.CASES.values()) == 129
    for name in tes.FULL:
        assert tes.base_of(name) + "@1" in tes.CASES and tes.CASES[tes.base_of(name) + "@1"].iters == 1
        assert (name in tes.CASES) == (name not in tes.AT_ONE_ONLY)
    assert set(tes.AT_ONE_ONLY) <= set(tes.FULL) and len(set(tes.AT_ONE_ONLY)) == len(tes.AT_ONE_ONLY)
    assert tes.NO_UNIQUE_BASIS == ("fundamental/rank1", "fundamental/nearequal", "fundamental/zero")
    for prefix in tes.NO_UNIQUE_BASIS:                     # ... and they are what the list says: coinciding singular values
        s = np.linalg.svd(tes.CASES[prefix + "@1"].x0, compute_uv=False)
        assert min(s[0] - s[1], s[1] - s[2]) <= 1.001e-3 * s[0], (prefix, s)
    for name, case in tes.CASES.items():
        if case.kind == "fundamental" and tes.has_unique_basis(name):
            s = np.linalg.svd(case.x0, compute_uv=False)
            assert min(s[0] - s[1], s[1] - s[2]) > 1e-4 * s[0], (name, s)


def test_scenes_reach_the_branches_they_are_named_for():
    eps = np.finfo(np.float64).eps
    x = {k: tes.CASES[f"angular/{k}/exact/trivial@1"].x0 for k in tes.ANGULAR_POSES}
    sigma = lambda p: p[3] * p[3] + p[4] * p[4]
    assert sigma(x["pole+"]) == 0.0 and x["pole+"][5] == 1.0 and sigma(x["pole-"]) == 0.0 and x["pole-"][5] == -1.0
    assert 0.0 < sigma(x["nearpole+"]) <= eps and x["nearpole+"][5] > 0.0            # inside householder3's branch, beta = 0
    assert 0.0 < sigma(x["nearpole-"]) <= eps and x["nearpole-"][5] < 0.0            # ... beta = 2
    assert sigma(x["south"]) > eps and x["south"][5] < 0.0                           # the x[2] <= 0 form of vp
    assert not x["rot0"][:3].any()
    assert 0.0 < x["rot5e-9"][:3] @ x["rot5e-9"][:3] <= eps < x["rot1e-7"][:3] @ x["rot1e-7"][:3] < 1e-13
    assert abs(np.linalg.norm(x["rotpi"][:3]) - (np.pi - 1e-3)) < 1e-15
    # clamped and valid residuals in one problem, at the start and for every loss
    case = tes.CASES["angular/clamped-mix/exact/trivial@1"]
    r = ref.Angular(case.corr, case.loss, case.width).raw(case.x0).reshape(-1)
    assert 5 <= int((r == 1000.0).sum()) <= 60 and case.n == 65, int((r == 1000.0).sum())
    H = {k: tes.CASES[f"homography/{k}/trivial@1"].x0 for k in ("x1e8", "x1e-8", "negated", "h22zero", "singular")}
    assert abs(H["x1e8"][2, 2]) > 1e7 and abs(H["x1e-8"][2, 2]) < 1e-7 and H["negated"][2, 2] < 0.0 and H["h22zero"][2, 2] == 0.0
    assert np.linalg.det(H["singular"]) == 0.0 and np.linalg.matrix_rank(H["h22zero"]) == 3
    F = {k: tes.CASES[f"fundamental/{k}@1"].x0 for k in ("n65", "negated", "x1e6", "fullrank", "rank1", "nearequal", "zero")}
    assert np.array_equal(F["negated"], -F["n65"]) and np.array_equal(F["x1e6"], 1e6 * F["n65"]) and not F["zero"].any()
    assert np.linalg.matrix_rank(F["n65"], tol=1e-12) == 2 and np.linalg.matrix_rank(F["fullrank"], tol=1e-6) == 3
    assert np.linalg.matrix_rank(F["rank1"], tol=1e-12) == 1
    assert np.allclose(np.linalg.svd(F["nearequal"], compute_uv=False), [1.0, 0.999, 0.0], atol=1e-15)


def test_independent_residuals_vanish_on_noise_free_data():
    """fixes the conventions of the generator: x2 ~ R(w) (X - t), H x1 ~ x2, x2' F x1 = 0"""
    seen = set()
    for name, case in tes.FULL.items():
        key = (case.kind, case.clean.tobytes())
        if case.n == 0 or key in seen:
            continue
        seen.add(key)
        P = PROBLEM[case.kind](case.clean, tes.TRIVIAL, 1.0)
        r, _ = P.evaluate(case.truth, False)
        scale = 1.0 if case.kind == "angular" else np.abs(case.clean).max()       # pixels, squared pixels
        assert np.abs(r).max() <= 1e-11 * scale, (name, np.abs(r).max())
    assert len(seen) >= 40


@pytest.mark.parametrize("kind", KINDS)
def test_every_at_one_form_is_admitted(kind):
    for name in at_one(kind):
        assert admitted(tes.CASES[name], oracle(name)), name


def test_at_one_only_is_exactly_the_unadmitted_set():
    unadmitted = [name for name, case in tes.FULL.items() if not admitted(case, tes.solve_oracle(case))]
    assert sorted(unadmitted) == sorted(tes.AT_ONE_ONLY)


@pytest.mark.parametrize("kind", KINDS)
def test_oracle_first_step_is_the_independent_step(kind):
    worst = (0.0, "")
    for name in filter(compares_step, at_one(kind)):
        case = tes.CASES[name]
        x, s = oracle(name)
        x_ref, _, accepted, iterations = independent(name)
        assert s["num_successful_steps"] == int(accepted) and s["num_iterations"] == iterations, (name, s, accepted, iterations)
        d = step_deviation(case, x, x_ref)
        worst = max(worst, (d, name))
        assert d <= STEP_BOUND[kind], (name, d)
    print(f"{kind}: largest deviation of the oracle's first step from the independent one {worst[0]:.3e} ({worst[1]}), bound {STEP_BOUND[kind]:.1e}")
    assert worst[1]


@pytest.mark.parametrize("kind", KINDS)
def test_oracle_initial_cost_is_the_long_double_sum(kind):
    worst = (0.0, "")
    for name in at_one(kind):
        case = tes.CASES[name]
        _, s = tes.solve_oracle(case.at(0))
        assert s["num_iterations"] == 0 and s["num_successful_steps"] == 0, name
        want = ref.initial_cost_longdouble(PROBLEM[case.kind](case.corr, case.loss, case.width), case.x0)
        if not np.isfinite(want):
            assert not np.isfinite(s["initial_cost"]), name
            continue
        d = abs(s["initial_cost"] - want) / want if want else abs(s["initial_cost"])
        worst = max(worst, (d, name))
        assert d <= INITIAL_COST_BOUND, (name, d)
    print(f"{kind}: largest relative deviation of the initial cost {worst[0]:.3e} ({worst[1]}), bound {INITIAL_COST_BOUND:.1e}")


def test_failure_and_empty_paths():
    for name, case in tes.CASES.items():
        x, s = oracle(name)
        label = name.split("/")[1].split("@")[0]
        if case.n == 0:                                     # the three agree; F included (it used to FAIL after 5 invalid steps)
            assert (s["termination_type"], s["success"], s["num_iterations"], s["num_successful_steps"]) == (tes.CONVERGENCE, 1, 0, 0), (name, s)
            assert s["initial_cost"] == 0.0 and s["final_cost"] == 0.0, (name, s)
            want = case.x0 / case.x0[2, 2] if case.kind == "homography" else case.x0
            assert np.array_equal(x, want), name
        elif (case.kind, label) in (("homography", "singular"), ("fundamental", "zero")):
            assert (s["termination_type"], s["success"], s["num_iterations"], s["num_successful_steps"]) == (tes.FAILURE, 0, 0, 0), (name, s)
            assert not np.isfinite(s["initial_cost"]), (name, s)
            assert np.array_equal(x, case.x0), name         # singular H0 has H(2, 2) = 1
        else:
            assert s["termination_type"] != tes.FAILURE and s["success"] == 1 and np.isfinite(s["initial_cost"]), (name, s)
            assert s["final_cost"] <= s["initial_cost"], (name, s)
