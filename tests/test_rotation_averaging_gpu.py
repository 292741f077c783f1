"""GPU: theia_hip_robust_rotation_averaging against the numpy restatement (tests/rotation_averaging_ref.py), the
factor-once multi-right-hand-side Cholesky against numpy, and the C-ABI's refusals."""
import ctypes as C

import numpy as np
import pytest

from pytheiasfm_amd import _capi as capi
from pytheiasfm_amd import global_pose, sfm
from tests import k3_systems as k3s
from tests import rotation_averaging_ref as ref
from tests import rotation_scenes as rs

pytestmark = pytest.mark.gpu

# name: (views, pairs, noise in degrees, outlier fraction, fixed views, duplicate / reversed edges, seed, tolerance in degrees)
CASES = {
    "tiny_no_noise": (4, 6, 0.0, 0.0, 1, 0, 1, 1e-8),
    "tiny_noise": (4, 6, 1.0, 0.0, 1, 0, 1, 1.0),
    "tiny_two_fixed": (4, 6, 2.0, 0.0, 2, 0, 1, 5.0),
    "v100": (100, 800, 2.0, 0.0, 1, 0, 1, 5.0),
    "v100_five_fixed": (100, 800, 2.0, 0.0, 5, 0, 1, 5.0),
    "v300_outliers": (300, 3000, 2.0, 0.1, 1, 0, 1, 5.0),
    "v60_duplicate_reversed": (60, 500, 2.0, 0.1, 1, 25, 1, 5.0),
    "v2000_outliers": (2000, 30000, 2.0, 0.1, 3, 0, 1, 5.0),
}


def _scene(name):
    n, pairs, noise, out, nfix, dup, seed, tol = CASES[name]
    s = rs.make_scene(n, pairs, noise, out, seed=seed)
    if dup:
        s = rs.with_duplicates(s, dup, dup, seed=seed)
    return s, np.arange(n) < nfix, tol


@pytest.mark.parametrize("name", list(CASES))
def test_matches_the_restatement(name):
    s, fixed, tol = _scene(name)
    r = ref.robust_rotation_averaging(s["init"], s["edges"], s["rel"], fixed)
    # equal iteration counts only mean something when no convergence decision of the restatement is a near tie
    assert min(m for _, m in r["margins"]) > 1e-6
    rc, got, summ = global_pose.robust_rotation_averaging(s["init"], s["edges"], s["rel"], fixed)
    assert rc == 0, capi.lib().theia_hip_last_error()
    assert (summ.l1_iterations, summ.admm_iterations, summ.irls_iterations) == (
        r["l1_iterations"], r["admm_iterations"], r["irls_iterations"])
    assert rs.angle_between(got, r["orientations"]).max() <= 1e-8
    assert np.array_equal(got[fixed], s["init"][fixed])
    assert rs.aligned_errors_deg(got, s["gt"]).max() < tol
    assert abs(summ.final_squared_residual - r["final_squared_residual"]) <= 1e-8 * max(1.0, r["final_squared_residual"])
    rc2, again, summ2 = global_pose.robust_rotation_averaging(s["init"], s["edges"], s["rel"], fixed)
    assert rc2 == 0 and np.array_equal(again, got)   # bit-identical
    assert summ2.admm_iterations == summ.admm_iterations and summ2.final_squared_residual == summ.final_squared_residual


def test_mirror_api_and_object_state():
    """pyTheia's calling sequence: dict in, dict out; the default fixed view is the first key and stays fixed; the
    constraints of a second EstimateRotations call are added to the first call's (the restatement sees them twice)."""
    from pytheiasfm_amd.twoview import TwoViewInfo
    s = rs.make_scene(30, 150, 2.0, seed=4)
    ids = [10 * i + 3 for i in range(30)]
    pairs = {}
    for (a, b), r in zip(s["edges"], s["rel"]):
        info = TwoViewInfo(); info.rotation_2 = r.copy()
        pairs[(ids[a], ids[b])] = info
    orient = {ids[i]: s["init"][i].copy() for i in range(30)}
    est = sfm.RobustRotationEstimator(sfm.RobustRotationEstimatorOptions())
    out = est.EstimateRotations(pairs, orient)
    assert list(out) == ids and est.last_success
    r = ref.robust_rotation_averaging(s["init"], s["edges"], s["rel"])
    assert rs.angle_between(np.array([out[v] for v in ids]), r["orientations"]).max() <= 1e-8
    assert np.array_equal(orient[ids[0]], s["init"][0])   # the input dict is not modified
    # second call: constraints accumulate, view ids[0] stays fixed even though the dict now starts elsewhere
    orient2 = {v: out[v] for v in ids[5:] + ids[:5]}
    out2 = est.EstimateRotations(pairs, orient2)
    twice_e = np.concatenate([s["edges"], s["edges"]])
    twice_r = np.concatenate([s["rel"], s["rel"]])
    start = np.array([out[v] for v in ids])
    r2 = ref.robust_rotation_averaging(start, twice_e, twice_r, np.arange(30) == 0)
    assert np.array_equal(out2[ids[0]], out[ids[0]])
    assert rs.angle_between(np.array([out2[v] for v in ids]), r2["orientations"]).max() <= 1e-8


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_multi_rhs_solve_against_numpy(n):
    rng = np.random.default_rng(n + 17)
    M = rng.standard_normal((n, n + 8))
    A = M @ M.T + n * np.eye(n)
    L = capi.lib()
    for k in (1, 3):
        B = np.ascontiguousarray(rng.standard_normal((k, n)))
        X = np.empty((k, n))
        Al = np.ascontiguousarray(np.tril(A))
        capi.check(L.theia_hip_dense_spd_solve_multi(n, capi.ptr(Al, C.c_double), k, capi.ptr(B, C.c_double),
                                                      capi.ptr(X, C.c_double)))
        Xr = np.linalg.solve(A, B.T).T
        assert np.abs(X - Xr).max() <= 1e-12 * np.abs(Xr).max()
        assert max(k3s.eta(A, X[i], B[i]) for i in range(k)) <= k3s.eta_bound(n)   # backward error, long-double residual
        if k == 1:
            x1 = np.empty(n)
            b1 = np.ascontiguousarray(B[0])
            capi.check(L.theia_hip_dense_spd_solve(n, capi.ptr(Al, C.c_double), capi.ptr(b1, C.c_double), capi.ptr(x1, C.c_double)))
            assert np.abs(X[0] - x1).max() <= 1e-13 * np.abs(x1).max()


def test_multi_rhs_solve_refuses_an_indefinite_matrix():
    n = 65
    rng = np.random.default_rng(5)
    M = rng.standard_normal((n, n))
    A = M @ M.T + np.eye(n)
    A[40, 40] = -1.0
    Al = np.ascontiguousarray(np.tril(A))
    B = np.ones((3, n))
    X = np.empty((3, n))
    rc = capi.lib().theia_hip_dense_spd_solve_multi(n, capi.ptr(Al, C.c_double), 3, capi.ptr(B, C.c_double), capi.ptr(X, C.c_double))
    assert rc == capi.THEIA_HIP_ERR_INTERNAL


def test_refusals_leave_the_orientations_untouched():
    s = rs.make_scene(20, 60, 2.0, seed=9)
    aa = np.ascontiguousarray(s["init"].copy())
    # a second component (views 20, 21) without a fixed view
    init = np.concatenate([aa, np.array([[0.1, 0.0, 0.0], [0.0, 0.2, 0.0]])])
    edges = np.concatenate([s["edges"], [[20, 21]]]).astype(np.int32)
    rel = np.concatenate([s["rel"], [[0.0, 0.0, 0.1]]])
    for e, r, f, n in [(edges, rel, None, 22),                                           # component without a fixed view
                       (np.concatenate([s["edges"], [[3, 20]]]).astype(np.int32), rel, None, 20),   # edge out of range
                       (np.concatenate([s["edges"], [[-1, 2]]]).astype(np.int32), rel, None, 20),   # negative index
                       (s["edges"][:0], s["rel"][:0], None, 20)]:                        # no constraint
        orient = np.ascontiguousarray(init[:n].copy())
        before = orient.copy()
        summ = capi.RotationSummary()
        o = sfm.RobustRotationEstimatorOptions().to_c()
        ee = np.ascontiguousarray(e)
        rr = np.ascontiguousarray(r[: len(e)])
        rc = capi.lib().theia_hip_robust_rotation_averaging(n, capi.ptr(orient, C.c_double), capi.ptr(f, C.c_uint8), len(ee),
                                                             capi.ptr(ee, C.c_int32), capi.ptr(rr, C.c_double),
                                                             C.byref(o), C.byref(summ))
        assert rc == capi.THEIA_HIP_ERR_INVALID_ARGUMENT
        assert np.array_equal(orient, before)
    # a fixed id that is not a view: refused by the mirror before any call
    est = sfm.RobustRotationEstimator(sfm.RobustRotationEstimatorOptions())
    est.SetFixedGlobalRotations({0, 99})
    for (a, b), r in zip(s["edges"], s["rel"]):
        est.AddRelativeRotationConstraint((int(a), int(b)), r)
    with pytest.raises(capi.TheiaHipError) as ex:
        est.EstimateRotations({}, {i: aa[i] for i in range(20)})
    assert ex.value.code == capi.THEIA_HIP_ERR_INVALID_ARGUMENT
    # the component check is what the fixed flags decide: fixing view 20 makes the same graph solvable
    f = np.zeros(22, dtype=bool); f[0] = True; f[20] = True
    rc, got, _ = global_pose.robust_rotation_averaging(init, edges, rel, f)
    assert rc == 0 and np.array_equal(got[20], init[20])
