"""CPU: the numpy restatement of RobustRotationEstimator against the reference test's cases
(robust_rotation_estimator_test.cc:167-220), its Kronecker-form solves against the reference's 3N x 3N sparse form, and
the Python mirror's names and defaults against pyTheia's (sfm.cc:1749-1780)."""
import math

import numpy as np
import pytest

from tests import rotation_averaging_ref as ref
from tests import rotation_scenes as rs

# (views, pairs, noise in degrees, tolerance in degrees, fixed views)
REFERENCE_CASES = {
    "SmallTestNoNoise": (4, 6, 0.0, 1e-8, 1),
    "SmallTestWithNoise": (4, 6, 1.0, 1.0, 1),
    "LargeTestWithNoise": (100, 800, 2.0, 5.0, 1),
    "SmallTestNoNoiseFixedViews": (4, 6, 2.0, 5.0, 2),
    "LargeTestWithNoiseFixedViews": (100, 800, 2.0, 5.0, 5),
}


@pytest.mark.parametrize("name", sorted(REFERENCE_CASES))
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_restatement_passes_the_reference_cases(name, seed):
    n, pairs, noise, tol, nfix = REFERENCE_CASES[name]
    s = rs.make_scene(n, pairs, noise, seed=seed)
    fixed = np.arange(n) < nfix
    r = ref.robust_rotation_averaging(s["init"], s["edges"], s["rel"], fixed, check_kron=True)
    assert rs.aligned_errors_deg(r["orientations"], s["gt"]).max() < tol
    # every linear solve agrees with the reference's own 3N x 3N sparse form
    assert r["kron_max_rel"] <= 1e-10
    assert np.array_equal(r["orientations"][fixed], s["init"][fixed])


def test_restatement_with_outliers_and_duplicate_edges():
    s = rs.with_duplicates(rs.make_scene(60, 500, 2.0, outlier_fraction=0.1, seed=7), 20, 20, seed=7)
    r = ref.robust_rotation_averaging(s["init"], s["edges"], s["rel"], check_kron=True)
    assert r["kron_max_rel"] <= 1e-10
    assert rs.aligned_errors_deg(r["orientations"], s["gt"]).max() < 5.0


def test_restatement_counts_and_margins_are_recorded():
    s = rs.make_scene(30, 150, 2.0, seed=3)
    r = ref.robust_rotation_averaging(s["init"], s["edges"], s["rel"])
    kinds = [k for k, _ in r["margins"]]
    assert kinds.count("admm") == r["admm_iterations"]
    assert kinds.count("l1") == r["l1_iterations"]
    assert kinds.count("irls") == r["irls_iterations"]
    assert 1 <= r["l1_iterations"] <= 5 and r["admm_iterations"] <= 155 and 1 <= r["irls_iterations"] <= 100


def test_rotation_conversions_round_trip():
    rng = np.random.default_rng(11)
    aa = rng.uniform(-1.0, 1.0, size=(500, 3)) * rng.uniform(0.0, 3.1, size=(500, 1))
    aa /= np.maximum(1.0, np.linalg.norm(aa, axis=1, keepdims=True) / 3.1)
    assert np.abs(ref.R_to_aa(ref.aa_to_R(aa)) - aa).max() < 1e-9
    R = ref.aa_to_R(aa)
    assert np.abs(np.einsum("nij,nkj->nik", R, R) - np.eye(3)).max() < 1e-14


def test_mirror_names_and_defaults_match_pytheia():
    from pytheiasfm_amd import global_pose, sfm
    o = sfm.RobustRotationEstimatorOptions()
    # robust_rotation_estimator.h:64-84
    assert o.max_num_l1_iterations == 5 and o.l1_step_convergence_threshold == 0.001
    assert o.max_num_irls_iterations == 100 and o.irls_step_convergence_threshold == 0.001
    assert o.irls_loss_parameter_sigma == math.radians(5.0)
    est = sfm.RobustRotationEstimator(o)
    for name in ("EstimateRotations", "AddRelativeRotationConstraint", "SetFixedGlobalRotations"):
        assert callable(getattr(est, name))
    # reconstruction_estimator_options.h:64-70
    assert [(t.name, int(t)) for t in sfm.GlobalRotationEstimatorType] == [
        ("ROBUST_L1L2", 0), ("NONLINEAR", 1), ("LINEAR", 2), ("LAGRANGE_DUAL", 3), ("HYBRID", 4)]
    assert global_pose.RobustRotationEstimator is sfm.RobustRotationEstimator


def test_mirror_refuses_on_the_host_before_any_launch():
    """The CHECK-class errors the mirror detects itself: no constraint, a fixed id without an orientation, an edge naming
    a view without an orientation.  None of them reaches the device."""
    from pytheiasfm_amd import _capi as capi, sfm
    from pytheiasfm_amd.twoview import TwoViewInfo
    est = sfm.RobustRotationEstimator(sfm.RobustRotationEstimatorOptions())
    orient = {0: np.zeros(3), 1: np.zeros(3)}
    with pytest.raises(capi.TheiaHipError) as ex:
        est.EstimateRotations({}, orient)
    assert ex.value.code == capi.THEIA_HIP_ERR_INVALID_ARGUMENT
    info = TwoViewInfo(); info.rotation_2 = np.array([0.0, 0.1, 0.0])
    est.SetFixedGlobalRotations({7})
    with pytest.raises(capi.TheiaHipError) as ex:
        est.EstimateRotations({(0, 1): info}, orient)
    assert ex.value.code == capi.THEIA_HIP_ERR_INVALID_ARGUMENT
    est2 = sfm.RobustRotationEstimator(sfm.RobustRotationEstimatorOptions())
    with pytest.raises(capi.TheiaHipError) as ex:
        est2.EstimateRotations({(0, 5): info}, orient)
    assert ex.value.code == capi.THEIA_HIP_ERR_INVALID_ARGUMENT
