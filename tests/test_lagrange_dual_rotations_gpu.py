"""GPU: theia_hip_lagrange_dual_rotations and the LAGRANGE_DUAL / HYBRID mirror against the numpy restatement
(tests/lagrange_dual_ref.py) on the scenes of tests/lagrange_dual_scenes.py.

Tolerance on Y and X = Y_0' Y.  Per scene and setting the restatement runs twice with gathered neighbour sums, in
ascending and in descending order; the spread s of X between the two is the arithmetic's own noise, and the bound is
100 s, never below 1e-12; a scene whose bound would exceed 1e-9 is not used.  After an escape X is compared against the
restatement run with two admissible directions v; the bound is 100 times their spread, never below 1e-12 and never
above 1e-6.  Measured on the CPU (the values the tests recompute): s between 0 and 2.1e-15 on the pinned BCM scenes and
the edge structures (bound 1e-12 everywhere); between the two directions 3.8e-8 (up10), 1.1e-7 (up12) and 3.5e-8 (up16),
all three at the cap of 1e-6: a BCM stopped by a relative change of 1e-14 in f is still some 1e-7 from its
critical point in Y, and one sweep more or less after an escape moves it by that much."""
import types

import numpy as np
import pytest

from pytheiasfm_amd import _capi as capi
from pytheiasfm_amd import global_pose as gp
from tests import lagrange_dual_ref as ref
from tests import lagrange_dual_scenes as sc
from tests.rotation_averaging_ref import aa_to_R

pytestmark = pytest.mark.gpu

END = {name: k for k, name in enumerate(gp.LAGRANGE_DUAL_END_STATES)}


def options(tolerance=1e-8, max_iterations=500, staircase=True, coloured=False, **kw):
    o = gp.SDPSolverOptions(max_iterations, tolerance)
    o.solver_type = gp.SDPSolverType.RIEMANNIAN_STAIRCASE if staircase else gp.SDPSolverType.RANK_DEFICIENT_BCM
    o.sweep_order = gp.SweepOrder.COLOURED if coloured else gp.SweepOrder.INDEX
    for k, v in kw.items():
        setattr(o.riemannian_staircase_options, k, v)
    return o


def run(name, opts, y_init=None):
    s = sc.scene(name)
    rc, aa, est, sm, Y, log = gp.lagrange_dual_rotations(s["n"], s["edges"], s["rel"], opts, y_init=y_init, want_y=True,
                                                         want_log=True)
    assert rc == 0, capi.lib().theia_hip_last_error()
    return aa, est, sm, Y, log


def bound_from_sums(name, **kw):
    spread, _, _ = sc.x_spread(name, **kw)
    bound = max(100.0 * spread, 1e-12)
    print(f"{name} {kw}: spread {spread:.2e}, bound {bound:.2e}")
    assert bound <= 1e-9, "the scene's own noise is too large: replace it"
    return bound


def check_bcm(name, tolerance, coloured, rank_init=0, staircase=False):
    kw = dict(tolerance=tolerance, max_iterations=20000, staircase=staircase, coloured=coloured, rank_init=rank_init)
    want = sc.reference(name, **kw)
    bound = bound_from_sums(name, **kw)
    y0 = sc.y_init(name, rank_init) if rank_init else None
    aa, est, sm, Y, log = run(name, options(tolerance, 20000, staircase, coloured), y0)
    lv = want["levels"][-1]
    dy, dx = np.abs(Y - want["Y"]).max(), np.abs(Y[:, :3].T @ Y - want["Y"][:, :3].T @ want["Y"]).max()
    print(f"  sweeps {sm.sweeps} (restatement {lv['sweeps']}), f {sm.f!r} ({want['f']!r}), |dY| {dy:.2e}, |dX| {dx:.2e}, "
          f"levels {sm.schedule_levels}, launches per sweep {sm.schedule_launches}")
    assert sm.sweeps == lv["sweeps"] and sm.total_iterations_num == want["total_iterations_num"]
    assert sm.final_rank == want["final_rank"] == Y.shape[0]
    assert dy <= bound and dx <= bound
    assert abs(sm.f - want["f"]) <= 1e-12 * abs(want["f"])
    assert np.abs(Y.reshape(Y.shape[0], -1, 3).transpose(1, 2, 0) @ Y.reshape(Y.shape[0], -1, 3).transpose(1, 0, 2)
                  - np.eye(3)).max() <= 1e-14
    return aa, est, sm, Y, log, want


@pytest.mark.parametrize("views", [12, 40])
@pytest.mark.parametrize("coloured", [False, True])
@pytest.mark.parametrize("tolerance", [1e-8, 1e-14])
def test_bcm_at_rank_3_from_zero(views, coloured, tolerance):
    name = sc.pinned_name(views, coloured, tolerance)
    aa, est, sm, Y, log, want = check_bcm(name, tolerance, coloured)
    assert sm.end_state == END["bcm"] and sm.num_levels == 1 and est.all()
    assert np.abs(aa_to_R(aa) - aa_to_R(want["orientations"])).max() <= 1e-9
    assert np.abs(aa[0]).max() == 0.0   # the gauge view comes out as the identity


@pytest.mark.parametrize("rank", [4, 6])
@pytest.mark.parametrize("coloured", [False, True])
def test_bcm_entered_through_y_init(rank, coloured):
    name = sc.pinned_name(10, coloured, 1e-8, rank)
    aa, est, sm, Y, log, want = check_bcm(name, 1e-8, coloured, rank_init=rank)
    assert Y.shape[0] == rank and log[0][0] == rank
    assert np.abs(aa_to_R(aa) - aa_to_R(want["orientations"])).max() <= 1e-9


@pytest.mark.parametrize("name,coloured", sc.STRUCTURE_CASES)
def test_edge_structures(name, coloured):
    s = sc.scene(name)
    m, _, live = sc.compact(s)
    kw = dict(tolerance=1e-8, max_iterations=500, staircase=True, coloured=coloured)
    want = sc.reference(name, **kw)
    bound = bound_from_sums(name, **kw)
    before = np.full((s["n"], 3), 7.5)
    rc, aa, est, sm = gp.lagrange_dual_rotations(s["n"], s["edges"], s["rel"], options(coloured=coloured),
                                                 orientations_out=before.copy())
    assert rc == 0
    _, _, _, Y, log = run(name, options(coloured=coloured))
    dx = np.abs(Y[:, :3].T @ Y - want["X"]).max()
    print(f"  levels {sm.schedule_levels}, launches {sm.schedule_launches}, sweeps {sm.sweeps} ({want['levels'][-1]['sweeps']}), |dX| {dx:.2e}")
    assert sm.end_state == END[want["end"]] == END["certified"] and sm.final_rank == 3
    assert sm.sweeps == want["levels"][-1]["sweeps"]
    assert dx <= bound
    assert sm.num_views_in_system == m and sm.gauge_view == live[0]
    assert est.tolist() == [v in set(live.tolist()) for v in range(s["n"])]
    assert (aa[~est] == 7.5).all()   # a view without an edge is left untouched
    assert np.abs(aa_to_R(aa[live]) - aa_to_R(want["orientations"])).max() <= 1e-9
    expected_levels = {"chain": (9, 2), "k8": (8, 8), "pair": (2, 2)}.get(name)
    if expected_levels:
        assert sm.schedule_levels == expected_levels[int(coloured)]


@pytest.mark.parametrize("key", [(12, False, 1e-8, 0), (40, True, 1e-8, 0), (10, False, 1e-8, 4)])
def test_certified_at_rank_3(key):
    name = sc.pinned_name(*key)
    want = sc.reference(name, coloured=key[1])
    aa, est, sm, Y, log = run(name, options(coloured=key[1]))
    S = ref.certificate_matrix(ref.build_problem(sm.num_views_in_system, sc.compact(sc.scene(name))[1], sc.scene(name)["rel"])[0], Y)
    lam = np.linalg.eigvalsh(S)[0]
    print(f"{name}: lambda_min of the device's Y by eigh {lam:.3e}, restatement {want['levels'][0]['lambda_min']:.3e}")
    assert (lam > -1e-5) and want["levels"][0]["certified"]
    assert sm.end_state == END["certified"] and log[0][3] == 1.0 and np.isnan(log[0][4]) and sm.factorisations == 1
    assert sm.final_rank == 3 and sm.sweeps == want["levels"][0]["sweeps"]


STAIRCASE = {"up10": (3, 4, 5), "up12": (3, 4, 5), "up16": (3, 4, 5, 6)}


@pytest.mark.parametrize("name", sorted(STAIRCASE))
def test_staircase_ascent(name):
    kw = dict(tolerance=1e-14, max_iterations=20000)
    w0, w1 = sc.reference(name, v_variant=0, **kw), sc.reference(name, v_variant=1, **kw)
    spread = np.abs(w0["X"] - w1["X"]).max()
    bound = min(max(100.0 * spread, 1e-12), 1e-6)
    print(f"{name}: spread between two admissible directions {spread:.2e}, bound {bound:.2e}")
    aa, est, sm, Y, log = run(name, options(1e-14, 20000))
    X = Y[:, :3].T @ Y
    for row, lv in zip(log, w0["levels"]):
        print(f"  rank {int(row[0])}: sweeps {int(row[1])} ({lv['sweeps']}), f {row[2]!r} ({lv['f']!r}), certified {row[3]}, "
              f"lambda_min {row[4]:.6e} ({lv['lambda_min']:.6e}), v'Sv {row[5]:.6e}, alpha {row[6]:.4f} ({lv['alpha']:.4f}), fallback {row[7]}")
    assert tuple(int(r[0]) for r in log) == tuple(lv["rank"] for lv in w0["levels"]) == STAIRCASE[name]
    for row, lv in zip(log, w0["levels"]):
        assert abs(row[2] - lv["f"]) <= 1e-9 * abs(lv["f"])
        assert bool(row[3]) == lv["certified"]
        if not lv["certified"]:   # the direction's quality, and the estimate the first step length is taken from
            assert row[5] <= 0.9 * lv["lambda_min"]
            # |d lambda_min| <= |d S| ~ |Q| |d Y|: the Y of two admissible paths differ by up to 1e-6, |Q| <= the degree
            assert abs(row[4] - lv["lambda_min"]) <= 1e-4
    assert sm.end_state == END["certified"] and sm.final_rank == STAIRCASE[name][-1] == Y.shape[0]
    # the rounded solution: the device's own Y through the restatement's rounding, and the restatement's result
    Xr, _ = ref.solution(Y, True)
    print(f"  |dX| before rounding {np.abs(X - (w0['Y'][:, :3].T @ w0['Y'])).max():.2e}, after {np.abs(Xr - w0['X']).max():.2e}")
    assert np.abs(Xr - w0["X"]).max() <= bound
    assert np.abs(aa_to_R(aa) - aa_to_R(w0["orientations"])).max() <= 10.0 * bound


@pytest.mark.parametrize("name", sorted(STAIRCASE))
def test_default_tolerance_on_the_staircase_scenes(name):
    aa, est, sm, Y, log = run(name, options())
    print(name, gp.LAGRANGE_DUAL_END_STATES[sm.end_state], [(int(r[0]), int(r[1]), r[2], r[4]) for r in log])
    assert sm.end_state in (END["certified"], END["max_rank"], END["escape_failed"])
    f = [r[2] for r in log] + [sm.f]
    assert all(b <= a for a, b in zip(f, f[1:]))
    assert np.isfinite(aa).all() and est.all()


def view_pairs_of(s, ids):
    return {(ids[a], ids[b]): types.SimpleNamespace(rotation_2=r.copy(), num_verified_matches=100 + k)
            for k, ((a, b), r) in enumerate(zip(s["edges"], s["rel"]))}


def test_hybrid_equals_stage_then_irls_and_lowers_the_robust_cost():
    s = sc.scene("v16out")
    ids = [10 + 3 * k for k in range(s["n"])]
    pairs = view_pairs_of(s, ids)
    start = {v: np.zeros(3) for v in ids}
    ld = gp.LagrangeDualRotationEstimator()
    stage = ld.EstimateRotations(pairs, start)
    hy = gp.HybridRotationEstimator()
    got = hy.EstimateRotations(pairs, start)
    want_stage = sc.reference("v16out")
    want = ref.irls_refine(want_stage["orientations"], s["edges"], s["rel"], gauge=0)
    a_stage, a_got = np.array([stage[v] for v in ids]), np.array([got[v] for v in ids])
    d_stage = np.abs(aa_to_R(a_stage) - aa_to_R(want_stage["orientations"])).max()
    d = np.abs(aa_to_R(a_got) - aa_to_R(want["orientations"])).max()
    c_stage, c_got = sc.robust_cost(a_stage, s["edges"], s["rel"]), sc.robust_cost(a_got, s["edges"], s["rel"])
    print(f"stage {d_stage:.2e}, hybrid {d:.2e}, irls iterations {hy.last_irls_summary.irls_iterations} "
          f"({want['irls_iterations']}), robust cost {c_stage:.6f} -> {c_got:.6f}")
    assert ld.gauge_view == ids[0] and ld.GetRASummary().end_state == END["certified"]
    assert d_stage <= 1e-9 and d <= 1e-8
    assert hy.last_success and hy.last_irls_summary.irls_iterations == want["irls_iterations"]
    assert hy.last_irls_summary.l1_iterations == 0
    assert c_got < c_stage
    assert all((start[v] == 0).all() for v in ids)


def test_from_the_maximum_spanning_tree_as_the_pipeline_calls_it():
    s = sc.scene(sc.pinned_name(12, False, 1e-8))
    ids = list(range(s["n"]))
    pairs = view_pairs_of(s, ids)
    seed = gp.OrientationsFromMaximumSpanningTree(pairs)
    got = gp.LagrangeDualRotationEstimator().EstimateRotations(pairs, seed)
    want = sc.reference(sc.pinned_name(12, False, 1e-8))
    assert sorted(got) == ids
    assert np.abs(aa_to_R(np.array([got[v] for v in ids])) - aa_to_R(want["orientations"])).max() <= 1e-9


def test_two_runs_give_identical_bytes():
    for name, o in (("up12", options(1e-14, 20000)), (sc.pinned_name(40, True, 1e-8), options(coloured=True))):
        a, b = run(name, o), run(name, o)
        assert a[0].tobytes() == b[0].tobytes() and a[3].tobytes() == b[3].tobytes() and a[4].tobytes() == b[4].tobytes()
        assert a[2].f == b[2].f and a[2].total_sweeps == b[2].total_sweeps


def refused(n, edges, rel, opts=None, y_init=None, code=capi.THEIA_HIP_ERR_INVALID_ARGUMENT):
    out = np.full((max(n, 0), 3), 3.25)
    rc, aa, est, sm = gp.lagrange_dual_rotations(n, edges, rel, opts, y_init=y_init, orientations_out=out)
    assert rc == code, (rc, capi.lib().theia_hip_last_error())
    assert (aa == 3.25).all() and not est.any() and sm.num_views_in_system == 0


def test_refusals():
    s = sc.scene("exact10")
    n, e, r = s["n"], s["edges"], s["rel"]
    refused(n, e[:0], r[:0])                                              # no edge
    bad = e.copy(); bad[3, 1] = n
    refused(n, bad, r)                                                    # a view out of range
    bad = e.copy(); bad[3, 0] = -1
    refused(n, bad, r)
    bad = e.copy(); bad[3] = (4, 4)
    refused(n, bad, r)                                                    # a self pair
    refused(n, np.vstack([e, e[2:3]]), np.vstack([r, r[2:3]]))            # a pair given twice
    refused(n, np.vstack([e, e[2:3, ::-1]]), np.vstack([r, r[2:3]]))      # ... in the other direction
    refused(6, np.array([(0, 1), (1, 2), (4, 5)]), r[:3])                 # two components
    for lo, hi in ((2, 10), (3, 11), (5, 4)):
        refused(n, e, r, options(min_rank=lo, max_rank=hi))
    for field in ("min_eigenvalue_nonnegativity_tolerance", "gradient_tolerance", "preconditioned_gradient_tolerance"):
        for value in (-1e-9, np.nan, np.inf):
            refused(n, e, r, options(**{field: value}))
    for value in (-1e-9, np.nan, np.inf):
        refused(n, e, r, options(tolerance=value))
    refused(n, e, r, options(max_iterations=0))
    refused(n, e, r, options(max_iterations=-3))
    for rank in (2, 11):
        refused(n, e, r, options(staircase=False), y_init=np.zeros((rank, 3 * n)))
    refused(n, e, r, options(max_rank=5), y_init=ref.project_blocks(np.ones((6, 3 * n)) + np.eye(6, 3 * n)))
    o = options()
    o.solver_type = gp.SDPSolverType.RBR_BCM
    refused(n, e, r, o, code=capi.THEIA_HIP_ERR_UNSUPPORTED)
    o.solver_type = gp.SDPSolverType.SHONAN
    refused(n, e, r, o)


def test_noise_free_scene_is_recovered():
    s = sc.scene("exact10")
    aa, est, sm, Y, log = run("exact10", options())
    # every pair contributes -2 tr(Y_i R_e' Y_j') = -2 tr(I_3) at the exact solution
    assert sm.end_state == END["certified"] and abs(sm.f + 6 * len(s["edges"])) <= 1e-12 * 6 * len(s["edges"])
    Rgt = aa_to_R(s["gt"])
    assert np.abs(aa_to_R(aa) - Rgt @ Rgt[0].T).max() <= 1e-12


@pytest.mark.parametrize("rank", [3, 5])
@pytest.mark.parametrize("ratio", [1e-1, 1e-2, 1e-3])
def test_polar_factor_down_to_the_stated_conditioning(rank, ratio):
    """A star entered through y_init and stopped after one sweep: the hub is updated first, from G_0 = -(Y_1 + Y_2) W of
    the start, W the relative rotation of both pairs.  Y_1 = P and Y_2 = P T with P a random block with orthonormal
    columns and T a turn about x by theta give G_0 the singular values 2, 2 cos(theta / 2), 2 cos(theta / 2) in general
    position, so sigma_min / sigma_max = cos(theta / 2) = ratio.  Bound on the factor: numpy's own error at this
    conditioning, eps / ratio, times 100."""
    rng = np.random.default_rng(77 + rank)
    theta = 2.0 * np.arccos(ratio)
    P = ref.polar(rng.normal(size=(rank, 3)))[0]
    w = sc.random_rotations(rng, 1)
    y0 = np.zeros((rank, 9))
    y0[:3, :3] = np.eye(3)
    y0[:, 3:6] = P
    y0[:, 6:9] = P @ aa_to_R(np.array([[theta, 0.0, 0.0]]))[0]
    o = options(1e-8, 1, staircase=False)
    rc, aa, est, sm, Y = gp.lagrange_dual_rotations(3, [(0, 1), (0, 2)], np.vstack([w, w]), o, y_init=y0, want_y=True)
    assert rc == 0 and sm.sweeps == 1
    # owner 0 is the pairs' first view: Q_j0 = -R_e, and Y_0 = the polar factor of -G_0
    want, sigma_min = ref.polar((y0[:, 3:6] + y0[:, 6:9]) @ aa_to_R(w)[0])
    got = Y[:, :3]
    print(f"rank {rank}, ratio {ratio}: sigma_min {sigma_min:.3e}, |d| {np.abs(got - want).max():.2e}, "
          f"|Y'Y - I| {np.abs(got.T @ got - np.eye(3)).max():.2e}")
    assert abs(sigma_min / 2.0 - ratio) <= 1e-12 * ratio + 1e-15
    assert np.abs(got.T @ got - np.eye(3)).max() <= 1e-14
    assert np.abs(got - want).max() <= 100.0 * np.finfo(float).eps / ratio
