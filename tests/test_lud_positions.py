"""CPU: the numpy restatement of LeastUnsquaredDeviationPositionEstimator against the reference test's cases
(least_unsquared_deviation_position_estimator_test.cc:218-251), its Schur-form solves against the full sparse form,
the held view's role, the Python mirror's names and defaults against pyTheia's (sfm.cc:1196-1204, 1707-1726), and the
refusals that happen before any launch."""
import ctypes as C

import numpy as np
import pytest

from tests import lud_positions_ref as ref
from tests import position_scenes as ps

# (views, pairs, noise in degrees, tolerance after alignment)
REFERENCE_CASES = {
    "SmallTestNoNoise": (4, 6, 0.0, 1e-2),
    "SmallTestWithNoise": (4, 6, 1.0, 0.1),
    "TestNoNoise": (200, 500, 0.0, 0.5),
    "TestWithNoise": (200, 500, 1.0, 1.0),
}


@pytest.mark.parametrize("name", sorted(REFERENCE_CASES))
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_restatement_passes_the_reference_cases(name, seed):
    n, pairs, noise, tol = REFERENCE_CASES[name]
    s = ps.make_scene(n, pairs, noise, seed=seed)
    r = ref.lud_positions(s["orientations"], s["edges"], s["rel"], check_schur=True)
    assert ps.aligned_errors(r["positions"], s["gt"]).max() < tol
    # every x-update agrees with the Schur form the device solves
    assert r["schur_max_rel"] <= 1e-10
    assert np.array_equal(r["positions"][0], np.zeros(3))
    assert len(r["margins"]) == r["admm_iterations"] and r["final_margins"] == r["margins"][-2:]


def test_schur_form_with_outliers_duplicates_and_held_views():
    s = ps.with_duplicates(ps.make_scene(40, 200, 2.0, outlier_fraction=0.1, seed=5), 10, 10, seed=5)
    fixed = np.arange(40) < 3
    o = ref.SolverOptions(max_num_iterations=300)
    full = ref.lud_positions(s["orientations"], s["edges"], s["rel"], fixed, o, check_schur=True)
    schur = ref.lud_positions(s["orientations"], s["edges"], s["rel"], fixed, o, form="schur")
    assert full["schur_max_rel"] <= 1e-10
    assert full["admm_iterations"] == schur["admm_iterations"]
    assert np.abs(full["positions"] - schur["positions"]).max() <= 1e-9 * ps.extent(full["positions"])
    assert not full["positions"][fixed].any()


def test_held_view_changes_positions_only_by_a_translation():
    """The column space of A does not depend on which view is held, so neither do the ADMM iterates A x, z, u.  The
    dual norms of the stopping test leave the held view's rows out, so the test runs to a fixed count here."""
    s = ps.make_scene(30, 120, 2.0, outlier_fraction=0.1, seed=8)
    o = ref.SolverOptions(max_num_iterations=150, absolute_tolerance=0.0, relative_tolerance=0.0)
    a = ref.lud_positions(s["orientations"], s["edges"], s["rel"], np.arange(30) == 0, o)
    b = ref.lud_positions(s["orientations"], s["edges"], s["rel"], np.arange(30) == 7, o)
    assert a["admm_iterations"] == b["admm_iterations"] == 150
    assert np.abs(b["positions"] - (a["positions"] - a["positions"][7])).max() <= 1e-9 * ps.extent(a["positions"])
    assert np.abs(b["scales"] - a["scales"]).max() <= 1e-9 * np.abs(a["scales"]).max()


def test_umeyama_recovers_a_similarity():
    rng = np.random.default_rng(3)
    src = rng.standard_normal((50, 3))
    th = 0.7
    R = np.array([[np.cos(th), -np.sin(th), 0.0], [np.sin(th), np.cos(th), 0.0], [0.0, 0.0, 1.0]])
    dst = 2.5 * src @ R.T + np.array([1.0, -2.0, 3.0])
    assert ps.aligned_errors(src, dst).max() < 1e-12


def test_mirror_names_and_defaults_match_pytheia():
    from pytheiasfm_amd import global_pose, sfm
    # reconstruction_estimator_options.h:80-85
    assert [(t.name, int(t)) for t in sfm.GlobalPositionEstimatorType] == [
        ("NONLINEAR", 0), ("LINEAR_TRIPLET", 1), ("LEAST_UNSQUARED_DEVIATION", 2), ("LIGT", 3)]
    # least_unsquared_deviation_position_estimator.h:60-69
    o = sfm.LeastUnsquaredDeviationPositionEstimatorOptions()
    assert (o.max_num_iterations, o.max_num_reweighted_iterations, o.convergence_criterion) == (400, 10, 1e-4)
    est = sfm.LeastUnsquaredDeviationPositionEstimator(o)
    assert callable(est.EstimatePositions)
    assert global_pose.LeastUnsquaredDeviationPositionEstimator is sfm.LeastUnsquaredDeviationPositionEstimator
    # what the estimator actually solves with: ConstrainedL1Solver::Options at their defaults (constrained_l1_solver.h:64-74)
    so = est.solver_options
    assert (so.max_num_iterations, so.rho, so.alpha, so.absolute_tolerance, so.relative_tolerance) == (1000, 10.0, 1.2, 1e-4, 1e-2)
    o.max_num_iterations = 5
    assert sfm.LeastUnsquaredDeviationPositionEstimator(o).solver_options.max_num_iterations == 1000
    c = so.to_c()
    assert (c.max_num_iterations, c.rho, c.alpha) == (1000, 10.0, 1.2)


def test_mirror_refuses_before_any_launch():
    """Empty input, a pair naming a view without an orientation and estimator options <= 0 are refused by the mirror;
    a disconnected graph, an edge out of range and solver options <= 0 by the C-ABI before the device is touched,
    with the positions untouched."""
    from pytheiasfm_amd import _capi as capi, global_pose, sfm
    from pytheiasfm_amd.twoview import TwoViewInfo
    est = sfm.LeastUnsquaredDeviationPositionEstimator(sfm.LeastUnsquaredDeviationPositionEstimatorOptions())
    orient = {0: np.zeros(3), 1: np.zeros(3), 2: np.zeros(3), 3: np.zeros(3)}
    info = TwoViewInfo(); info.position_2 = np.array([1.0, 0.0, 0.0])
    for pairs in ({}, {(0, 1): info, (1, 9): info}, {(0, 1): info, (2, 3): info}):
        with pytest.raises(capi.TheiaHipError) as ex:
            est.EstimatePositions(pairs, orient)
        assert ex.value.code == capi.THEIA_HIP_ERR_INVALID_ARGUMENT
    for field in ("max_num_iterations", "max_num_reweighted_iterations"):
        for bad in (0, -1):
            o = sfm.LeastUnsquaredDeviationPositionEstimatorOptions()
            setattr(o, field, bad)
            with pytest.raises(capi.TheiaHipError) as ex:
                sfm.LeastUnsquaredDeviationPositionEstimator(o)
            assert ex.value.code == capi.THEIA_HIP_ERR_INVALID_ARGUMENT

    s = ps.make_scene(10, 20, 1.0, seed=2)
    aa, e, t = s["orientations"], s["edges"], s["rel"]
    two = np.concatenate([aa, np.zeros((2, 3))])
    cases = [(two, np.concatenate([e, [[10, 11]]]), np.concatenate([t, [[1.0, 0.0, 0.0]]]), None),   # second component
             (aa, np.concatenate([e, [[3, 10]]]), np.concatenate([t, [[1.0, 0.0, 0.0]]]), None),     # out of range
             (aa, np.concatenate([e, [[-1, 2]]]), np.concatenate([t, [[1.0, 0.0, 0.0]]]), None),     # negative index
             (aa, e[:0], t[:0], None),                                                                # no pairs
             (aa, e, t, dict(max_num_iterations=0)), (aa, e, t, dict(rho=0.0)), (aa, e, t, dict(rho=-1.0))]
    for orient_a, edges, rel, bad in cases:
        so = global_pose.ConstrainedL1SolverOptions()
        for k, v in (bad or {}).items():
            setattr(so, k, v)
        out = np.full((orient_a.shape[0], 3), 7.25)
        rc, got, _ = global_pose.lud_positions(orient_a, edges, rel, None, so, positions_out=out)
        assert rc == capi.THEIA_HIP_ERR_INVALID_ARGUMENT
        assert got is out and np.all(out == 7.25)
    # a null summary pointer is refused as well
    o = global_pose.ConstrainedL1SolverOptions().to_c()
    pos = np.zeros((10, 3))
    ee = np.ascontiguousarray(e)
    rc = capi.lib().theia_hip_lud_positions(10, capi.ptr(np.ascontiguousarray(aa), C.c_double), None, len(ee),
                                            capi.ptr(ee, C.c_int32), capi.ptr(np.ascontiguousarray(t), C.c_double),
                                            C.byref(o), capi.ptr(pos, C.c_double), None)
    assert rc == capi.THEIA_HIP_ERR_INVALID_ARGUMENT
