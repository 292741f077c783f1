"""CPU: known answers of the LAGRANGE_DUAL restatement (tests/lagrange_dual_ref.py), the fairness of the scenes the GPU
tests run on (tests/lagrange_dual_scenes.py), and the mirror's names, defaults and host-side refusals."""
import math
import types

import numpy as np
import pytest

from pytheiasfm_amd import _capi as capi
from pytheiasfm_amd import global_pose as gp
from pytheiasfm_amd import sfm
from tests import lagrange_dual_ref as ref
from tests import lagrange_dual_scenes as sc
from tests.rotation_averaging_ref import aa_to_R


def test_noise_free_scene_is_recovered_exactly():
    s = sc.scene("exact10")
    for coloured in (False, True):
        w = sc.reference("exact10", coloured=coloured)
        # every pair contributes -2 tr(Y_i R_e' Y_j') = -2 tr(I_3) at the exact solution
        assert abs(w["f"] + 6 * len(s["edges"])) <= 1e-12 * 6 * len(s["edges"])
        assert w["end"] == "certified" and w["final_rank"] == 3
        Rgt = aa_to_R(s["gt"])
        assert np.abs(aa_to_R(w["orientations"]) - Rgt @ Rgt[0].T).max() <= 1e-12
        assert np.abs(w["orientations"][0]).max() == 0.0


def test_zero_start_gives_identity_over_zero():
    for rank in (3, 4, 7):
        P, sigma = ref.polar(np.zeros((rank, 3)))
        assert np.array_equal(P, np.eye(rank, 3)) and sigma == math.inf
    # the first view of a sweep from zero sees a zero G: its block is [I; 0], and its neighbours follow from it
    s = sc.scene("pair")
    Q, adj = ref.build_problem(2, s["edges"], s["rel"])
    Y, sweeps, f = ref.bcm(Q, adj, np.zeros((4, 6)), ref.Options(max_iterations=1))
    assert np.array_equal(Y[:, :3], np.eye(4, 3)) and sweeps == 1
    assert np.abs(Y[:3, 3:] - aa_to_R(s["rel"])[0].T).max() <= 1e-15 and abs(f + 6) <= 1e-14


def test_gathered_sums_and_levels_reproduce_the_sequential_sweep():
    for key in ((12, True, 1e-14, 0), (40, False, 1e-8, 0)):
        name = sc.pinned_name(*key)
        kw = dict(tolerance=key[2], max_iterations=20000, staircase=False, coloured=key[1])
        a, b = sc.reference(name, **kw), sc.reference(name, sums="ascending", **kw)
        assert a["levels"][0]["sweeps"] == b["levels"][0]["sweeps"]
        assert np.abs(a["Y"] - b["Y"]).max() <= 1e-13


@pytest.mark.parametrize("key", sorted(sc.PINNED))
def test_pinned_stopping_decisions_have_margin(key):
    views, coloured, tolerance, rank_init = key
    w = sc.reference(sc.pinned_name(*key), tolerance=tolerance, max_iterations=20000, staircase=False, coloured=coloured,
                     rank_init=rank_init)
    errs = w["record"]["errs"][0]
    assert errs[-1] <= tolerance / 4 and errs[-2] >= 4 * tolerance, errs[-2:]
    assert w["record"]["min_sigma"] >= 0.1
    spread, a, d = sc.x_spread(sc.pinned_name(*key), tolerance=tolerance, max_iterations=20000, staircase=False,
                               coloured=coloured, rank_init=rank_init)
    assert 100.0 * spread <= 1e-9
    assert a["levels"][0]["sweeps"] == d["levels"][0]["sweeps"] == w["levels"][0]["sweeps"]


@pytest.mark.parametrize("name,coloured", sc.STRUCTURE_CASES)
def test_structure_scenes_are_fair(name, coloured):
    w = sc.reference(name, coloured=coloured)
    errs = w["record"]["errs"][0]
    assert errs[-1] <= 0.8e-8 and errs[-2] >= 1.25e-8, errs[-2:]   # lagrange_dual_scenes.STRUCTURE_SEED has the reasoning
    assert w["record"]["min_sigma"] >= 0.1
    assert w["end"] == "certified" and w["levels"][0]["lambda_min"] >= -1e-6
    assert 100.0 * sc.x_spread(name, coloured=coloured)[0] <= 1e-9


def test_certificate_decisions_have_margin():
    seen = []
    for name in ("up10", "up12", "up16"):
        for variant in (0, 1):
            w = sc.reference(name, tolerance=1e-14, max_iterations=20000, v_variant=variant)
            assert w["end"] == "certified"
            seen += [lv["lambda_min"] for lv in w["levels"]]
            assert w["record"]["min_sigma"] >= 0.1
    for key in ((12, False, 1e-8, 0), (40, True, 1e-8, 0), (10, False, 1e-8, 4)):
        w = sc.reference(sc.pinned_name(*key), coloured=key[1])
        errs = w["record"]["errs"][0]
        assert errs[-1] <= 1e-8 / 4 and errs[-2] >= 4e-8
        seen += [lv["lambda_min"] for lv in w["levels"]]
    w = sc.reference("v16out")
    errs = w["record"]["errs"][0]
    assert errs[-1] <= 0.8e-8 and errs[-2] >= 1.25e-8 and w["end"] == "certified"
    seen += [lv["lambda_min"] for lv in w["levels"]]
    # the threshold is -1e-5: every decision lies a factor of 10 or more away from it
    assert all(lam <= -1e-3 or lam >= -1e-6 for lam in seen), seen
    assert sum(lam <= -1e-3 for lam in seen) >= 14


def test_staircase_paths_of_the_scenes():
    for name, ranks in (("up10", (3, 4, 5)), ("up12", (3, 4, 5)), ("up16", (3, 4, 5, 6))):
        w = sc.reference(name, tolerance=1e-14, max_iterations=20000)
        assert tuple(lv["rank"] for lv in w["levels"]) == ranks and w["final_rank"] == ranks[-1]
        f = [lv["f"] for lv in w["levels"]]
        assert all(b < a for a, b in zip(f, f[1:]))
        assert all(not lv["fallback"] for lv in w["levels"])


def test_mirror_names_and_defaults():
    o = sfm.SDPSolverOptions()
    assert (o.max_iterations, o.tolerance, o.verbose, o.num_threads) == (500, 1e-8, True, 8)
    assert o.solver_type == sfm.SDPSolverType.RIEMANNIAN_STAIRCASE and o.preconditioner_type == sfm.PreconditionerType.NONE
    assert sfm.SDPSolverOptions(20, 1e-3, False).max_iterations == 20
    r = o.riemannian_staircase_options
    assert isinstance(r, sfm.RiemannianStaircaseOptions)
    assert (r.min_rank, r.max_rank, r.max_eigen_solver_iterations, r.num_Lanczos_vectors) == (3, 10, 20, 20)
    assert (r.min_eigenvalue_nonnegativity_tolerance, r.gradient_tolerance, r.preconditioned_gradient_tolerance) == (1e-5, 1e-2, 1e-4)
    assert r.local_solver_type == sfm.SDPSolverType.RANK_DEFICIENT_BCM
    assert [(t.name, int(t)) for t in sfm.SDPSolverType] == [("RBR_BCM", 0), ("RANK_DEFICIENT_BCM", 1),
                                                             ("RIEMANNIAN_STAIRCASE", 2), ("SE_SYNC", 3), ("SHONAN", 4)]
    c = o.to_c()
    assert (c.solver_type, c.max_iterations, c.min_rank, c.max_rank, c.sweep_order) == (2, 500, 3, 10, 0)
    assert (c.tolerance, c.min_eigenvalue_nonnegativity_tolerance, c.gradient_tolerance, c.preconditioned_gradient_tolerance) == (1e-8, 1e-5, 1e-2, 1e-4)
    h = sfm.HybridRotationEstimatorOptions()
    assert isinstance(h.sdp_solver_options, sfm.SDPSolverOptions)
    i = h.irls_options
    assert (i.max_num_irls_iterations, i.irls_step_convergence_threshold, i.irls_loss_parameter_sigma) == (10, 0.001, math.radians(5.0))
    for cls in (sfm.LagrangeDualRotationEstimator, sfm.HybridRotationEstimator):
        assert callable(getattr(cls(), "EstimateRotations"))
    e = sfm.LagrangeDualRotationEstimator()
    e.SetRAOption(o)
    assert e.options is o and e.GetRASummary() is None
    assert gp.LAGRANGE_DUAL_END_STATES == ("bcm", "certified", "max_rank", "escape_failed")


def test_mirror_host_side_refusals():
    info = types.SimpleNamespace(rotation_2=np.zeros(3))
    for est in (sfm.LagrangeDualRotationEstimator(), sfm.HybridRotationEstimator()):
        with pytest.raises(capi.TheiaHipError):
            est.EstimateRotations({}, {0: np.zeros(3), 1: np.zeros(3)})          # no pair
        with pytest.raises(capi.TheiaHipError):
            est.EstimateRotations({(0, 1): info}, {})                           # no orientation
        with pytest.raises(capi.TheiaHipError):
            est.EstimateRotations({(0, 2): info}, {0: np.zeros(3), 1: np.zeros(3)})   # a pair names an unknown view
    with pytest.raises(ValueError):
        gp.lagrange_dual_rotations(3, [(0, 1), (1, 2)], np.zeros((3, 3)))       # one rotation per pair
    with pytest.raises(ValueError):
        gp.lagrange_dual_rotations(3, [(0, 1), (1, 2)], np.zeros((2, 3)), y_init=np.zeros((3, 6)))   # 3 views have edges
    with pytest.raises(ValueError):
        gp.lagrange_dual_rotations(3, [(0, 1)], np.zeros((1, 3)), orientations_out=np.zeros((2, 3)))
