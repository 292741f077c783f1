"""GPU: theia_hip_linear_rotations (csrc/linear_rotations.hip) against the numpy restatement
(tests/linear_rotation_ref.py) on the scenes of tests/linear_rotation_scenes.py.

The orientations are defined up to one common rotation on the right, so they are compared free of it: the angle between
R_i R_0^T of the device and of the eigh reference, at most 1e-8 rad for every view.  At the stop d <= 1e-10 and the
contraction per step is at most 0.2 (lambda_3 / lambda_4, tests/test_linear_rotations.py), so the subspace error is at
most 2.5e-11; a view's block has singular values of about 1 / sqrt(n), so its polar factor moves by at most about
2 sqrt(n) times that, 1.3e-9 at n = 700; comparing relative to view 0 doubles it.  1e-8 is also the bound of
tests/test_rotation_averaging_gpu.py.  The eigenvalues: the Ritz error is of second order in the subspace error and the
rounding floor is about 3n eps lambda_max, so 1e-9 lambda_max leaves four orders of margin.  The iteration counts may
differ by one from the restatement's: on v300out the step before the stop is only 1.3 x above the threshold."""
import types

import numpy as np
import pytest

from pytheiasfm_amd import _capi as capi
from pytheiasfm_amd import global_pose, sfm
from tests import linear_rotation_ref as ref
from tests import linear_rotation_scenes as ls
from tests import rotation_scenes as rs

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
_runs = {}


def run(name):
    """One library call per scene, shared by the tests (not to be modified)."""
    if name not in _runs:
        s = ls.graph(name)
        _runs[name] = global_pose.linear_rotations(s["n"], s["edges"], s["rel"], orientations_out=np.full((s["n"], 3), 7.0))
    return _runs[name]


def _numbers(summ):
    return (summ.iterations, summ.num_views_in_system, tuple(summ.eigenvalues), summ.subspace_change, summ.shift)


@pytest.mark.parametrize("name", ls.SCENES)
def test_matches_the_restatement(name):
    s, r, d = ls.scene(name)
    rc, got, est, summ = run(name)
    assert rc == 0, capi.lib().theia_hip_last_error()
    assert est.all() and summ.num_views_in_system == s["n"]
    w = r["eigenvalues"]
    angle = ref.gauge_free_angles(got, r["orientations"]).max()
    eig = np.abs(np.array(summ.eigenvalues) - w[:3]).max() / w[-1]
    print(f"{name}: gauge-free difference {angle:.3e} rad, iterations {summ.iterations} (restatement {d['iterations']}), "
          f"last step {summ.subspace_change:.3e}, eigenvalue difference {eig:.3e} lambda_max, shift {summ.shift:.3e}")
    assert angle <= 1e-8
    assert abs(summ.iterations - d["iterations"]) <= 1 and summ.iterations <= 20
    assert summ.subspace_change <= 1e-10
    assert eig <= 1e-9
    assert list(summ.eigenvalues) == sorted(summ.eigenvalues)
    assert summ.shift == (3 * s["n"] * EPS) * r["M"].diagonal().max()
    if name in ls.GT_BOUND_DEG:
        assert rs.aligned_errors_deg(got, s["gt"]).max() <= ls.GT_BOUND_DEG[name]


@pytest.mark.parametrize("name", ls.SCENES)
def test_bit_reproducible(name):
    s = ls.graph(name)
    rc, got, est, summ = run(name)
    rc2, again, est2, summ2 = global_pose.linear_rotations(s["n"], s["edges"], s["rel"])
    assert rc == 0 and rc2 == 0
    assert np.array_equal(again, got) and np.array_equal(est2, est)
    assert _numbers(summ2) == _numbers(summ)


def test_views_without_edges_are_left_alone():
    s = ls.graph("v22")
    rc, plain, _, summ = run("v22")
    out = np.full((24, 3), 7.0)
    rc2, got, est, summ2 = global_pose.linear_rotations(24, s["edges"], s["rel"], orientations_out=out)
    assert rc == 0 and rc2 == 0
    assert np.all(got[22:] == 7.0) and list(est) == [True] * 22 + [False] * 2
    assert np.array_equal(got[:22], plain)                 # bit for bit
    assert summ2.num_views_in_system == 22 and _numbers(summ2) == _numbers(summ)
    # the same with the two views in front: the system's indices are compact in view order
    out = np.full((24, 3), 7.0)
    rc3, moved, est3, _ = global_pose.linear_rotations(24, s["edges"] + 2, s["rel"], orientations_out=out)
    assert rc3 == 0 and np.all(moved[:2] == 7.0) and not est3[:2].any() and np.array_equal(moved[2:], plain)


def test_one_iteration_is_no_convergence():
    s = ls.graph("v100")
    o = global_pose.LinearRotationEstimatorOptions()
    o.max_num_iterations = 1
    rc, got, est, summ = global_pose.linear_rotations(s["n"], s["edges"], s["rel"], o)
    assert rc == capi.THEIA_HIP_ERR_INTERNAL
    assert "no convergence" in capi.lib().theia_hip_last_error().decode()
    assert summ.iterations == 1 and summ.subspace_change > 1e-10
    assert np.isfinite(got).all() and est.all() and np.isfinite(list(summ.eigenvalues)).all()


def test_python_class_against_the_array_call():
    s = rs.make_scene(30, 150, 2.0, seed=4)
    ids = [10 * i + 3 for i in range(30)]
    pairs = {(ids[a], ids[b]): types.SimpleNamespace(rotation_2=r.copy()) for (a, b), r in zip(s["edges"], s["rel"])}
    est = sfm.LinearRotationEstimator()
    out = est.EstimateRotations(pairs)
    assert list(out) == ids                                # the chain edges name the views in order
    assert est.last_success is True and est.last_summary.num_views_in_system == 30
    rc, direct, _, _ = global_pose.linear_rotations(30, s["edges"], s["rel"])
    assert rc == 0
    assert ref.gauge_free_angles(np.array([out[v] for v in ids]), direct).max() <= 1e-8
    r = ref.reference(30, s["edges"], s["rel"])
    assert ref.gauge_free_angles(direct, r["orientations"]).max() <= 1e-8
