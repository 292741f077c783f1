"""GPU: the Jacobi scaling folded into the first linearisation of a BA solve (k_lin_schur's first-launch instance, the
camera scales from that launch's column norms, the rescaled reduced system) against the separate column-norm pass
(THEIA_HIP_SCALE_PASS=1) and against the CPU oracle.

The problems are synth_ba_v1(30, 2500) with mixed pinhole / double-sphere groups, some tracks lengthened to 11 .. 22
cameras (22 variable cameras is the most the fused plan takes in a track), partly and wholly constant cameras and constant
points.  Each problem is solved once per route in a fresh handle, and once by the oracle (shared by the tests of a case).
Bounds against the oracle: those of test_ba_gpu.test_lm_trajectory_matches_oracle_c1; route against route: 1e-9 on the
cost and radius traces.  The figures are printed before they are asserted (pytest -s).

Why the robust loss rides the tangent-space (PD 3) problem and the ambient (PD 4) problem has the trivial loss: with PD 4 the
homogeneous scale of a point is a gauge direction that only the LM diagonal damps.  The Huber solve of this problem ends at a
trust-region radius of 1.4e11, and there the ORACLE's own final points move by 5.5e-6 when its input is perturbed by 1e-15
relative (3.6e-9 as X / w, 4e-11 in the cameras), so the 1e-8 bound on the raw homogeneous points is below the reference's own
error for that combination, on either route.  The same perturbation moves the oracle's points by 2.4e-12 (PD 4, trivial loss,
radius 9e4), 6e-14 (PD 3, Huber) and 7e-14 (PD 3, rejected step): those cases carry the bound."""
import functools
import os

import numpy as np
import pytest

from pytheiasfm_amd import ba, synth
from tests import oracle_lib as ol

pytestmark = pytest.mark.gpu

SWITCH = "THEIA_HIP_SCALE_PASS"

# name: (seed, tangent-space points, loss type, loss width, inner iterations, start perturbation scale)
CASES = {
    "pd3_trivial_inner": (0x5CA1E001, 1, 0, 1.0, 1, 1.0),
    "pd4_trivial": (0x5CA1E002, 0, 0, 1.0, 0, 1.0),
    "pd3_huber": (0x5CA1E002, 1, 1, 1.5, 0, 1.0),
    "pd3_rejected_step": (0x5CA1E005, 1, 0, 1.0, 0, 6.0),   # (found with the oracle: the first step is rejected)
}


def rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def build_problem(seed, perturb):
    """synth_ba_v1(30, 2500), every 7th track lengthened to 11 .. 22 consecutive cameras of the ring (exact projections of
    the true point plus the generator's pixel noise level), constant cameras of every kind, every 5th point constant."""
    nv, nt = 30, 2500
    p, cam_gt, pts_gt = synth.synth_ba_v1(nv, nt, seed=seed, mixed_models=True, sigma_pos=0.05 * perturb,
                                          sigma_rot_deg=0.5 * perturb, sigma_pt=0.02 * perturb, return_truth=True)
    rng = np.random.default_rng(seed)
    first = np.full(nt, -1, np.int64); count = np.zeros(nt, np.int64)
    for i, t in enumerate(p.obs_pt):
        if first[t] < 0:
            first[t] = i
        count[t] += 1
    add_cam, add_pt = [], []
    for t in range(0, nt, 7):
        want = 11 + (t // 7) % 12
        w0 = p.obs_cam[first[t]]
        for k in range(count[t], want):
            add_cam.append((w0 + k) % nv); add_pt.append(t)
    add_cam = np.asarray(add_cam, np.int32); add_pt = np.asarray(add_pt, np.int32)
    uv = np.zeros((len(add_cam), 2))
    for m in np.unique(p.group_model):
        mm = p.group_model[p.cam_group[add_cam]] == m
        if mm.any():
            uv[mm], ok = synth.project(m, p.intrinsics[p.cam_group[add_cam[mm]]], cam_gt[add_cam[mm]], pts_gt[add_pt[mm]])
            assert ok.all()
    uv += 0.5 * rng.standard_normal(uv.shape)
    p.obs_uv = np.ascontiguousarray(np.vstack([p.obs_uv, uv]))
    p.obs_cam = np.ascontiguousarray(np.concatenate([p.obs_cam, add_cam]).astype(np.int32))
    p.obs_pt = np.ascontiguousarray(np.concatenate([p.obs_pt, add_pt]).astype(np.int32))
    cc = np.zeros(nv, np.uint8)
    cc[0] = 3; cc[5] = 1; cc[11] = 2; cc[17] = 4; cc[23] = 3   # whole block, position, rotation, tz, whole block
    p.cam_const = cc
    pc = np.zeros(nt, np.uint8); pc[::5] = 1
    p.point_const = pc
    return p


def case_options(name):
    _, manifold, loss, width, inner, _ = CASES[name]
    o, oo = ba.default_options(), ol.default_options()
    for x in (o, oo):
        x.use_homogeneous_point_parametrization = manifold
        x.loss_function_type = loss; x.robust_loss_width = width
        x.use_inner_iterations = inner
    return o, oo


@functools.lru_cache(maxsize=None)
def case_problem(name):
    return build_problem(CASES[name][0], CASES[name][5])


@functools.lru_cache(maxsize=None)
def oracle_solve(name):
    po = case_problem(name).copy()
    s, tr = ol.solve(po, case_options(name)[1])
    return po, s, tr


def gpu_solve(problem, options, separate_pass):
    """One solve in a fresh handle on the chosen route; the switch is read by every run()."""
    old = os.environ.pop(SWITCH, None)
    if separate_pass:
        os.environ[SWITCH] = "1"
    try:
        pg = problem.copy()
        s, tr = ba.solve(pg, options)
    finally:
        os.environ.pop(SWITCH, None)
        if old is not None:
            os.environ[SWITCH] = old
    return pg, s, tr


@functools.lru_cache(maxsize=None)
def route_solve(name, separate_pass):
    return gpu_solve(case_problem(name), case_options(name)[0], separate_pass)


def same_bits(a, b):
    (pa, sa, ta), (pb, sb, tb) = a, b
    return (np.array_equal(pa.cam_ext, pb.cam_ext) and np.array_equal(pa.points, pb.points) and ta.size == tb.size and
            np.array_equal(ta.cost, tb.cost) and np.array_equal(ta.radius, tb.radius) and np.array_equal(ta.accepted, tb.accepted) and
            np.array_equal(ta.gradient_max_norm, tb.gradient_max_norm) and np.array_equal(ta.step_norm, tb.step_norm))


@pytest.mark.parametrize("name", list(CASES))
def test_the_problem_takes_the_fused_plan_in_several_runs(name):
    p = case_problem(name)
    lengths = np.bincount(p.obs_pt)
    assert lengths.min() == 2 and lengths.max() == 22
    with ba.BaHandle(p.copy(), case_options(name)[0]) as h:
        info = h.plan_info()
    print(name, "plan:", info)
    assert info["slow_path_tracks"] == 0 and info["fused_runs"] >= 2


@pytest.mark.parametrize("separate_pass", [False, True], ids=["folded", "separate_pass"])
@pytest.mark.parametrize("name", list(CASES))
def test_each_route_matches_the_oracle(name, separate_pass):
    pg, s, tr = route_solve(name, separate_pass)
    po, so, tro = oracle_solve(name)
    print(name, "separate pass" if separate_pass else "folded", "iterations", s.num_iterations, "accepted", tro.accepted[: tro.size].tolist(),
          "rel cost %.3e" % rel(tr.cost, tro.cost), "rel radius %.3e" % rel(tr.radius, tro.radius),
          "gradient %.3e" % (np.abs(tr.gradient_max_norm - tro.gradient_max_norm).max() / tro.gradient_max_norm.max()),
          "rel step %.3e" % rel(tr.step_norm, tro.step_norm), "cam %.3e" % np.abs(pg.cam_ext - po.cam_ext).max(),
          "points %.3e" % np.abs(pg.points - po.points).max())
    assert s.success == so.success == 1 and s.termination_type == so.termination_type
    assert s.num_iterations == so.num_iterations and tr.size == tro.size
    assert np.array_equal(tr.accepted, tro.accepted)
    assert rel(tr.cost, tro.cost) <= 1e-9 and rel(tr.radius, tro.radius) <= 1e-9
    assert np.abs(tr.gradient_max_norm - tro.gradient_max_norm).max() <= 1e-6 * tro.gradient_max_norm.max()
    assert rel(tr.step_norm, tro.step_norm) <= 1e-6
    assert abs(s.initial_cost - so.initial_cost) <= 1e-12 * so.initial_cost
    assert abs(s.final_cost - so.final_cost) <= 1e-9 * so.final_cost
    assert np.abs(pg.cam_ext - po.cam_ext).max() <= 1e-8 and np.abs(pg.points - po.points).max() <= 1e-8
    p = case_problem(name)
    assert np.array_equal(pg.cam_ext[[0, 23]], p.cam_ext[[0, 23]]) and np.array_equal(pg.points[::5], p.points[::5])


def test_the_rejected_step_case_rejects_a_step_early():
    _, _, tro = oracle_solve("pd3_rejected_step")
    assert tro.accepted[0] == 1 and 0 in tro.accepted[1:4].tolist()   # (entry 0 is the start; 1 .. 3 the first three steps)


@pytest.mark.parametrize("name", list(CASES))
def test_the_two_routes_agree(name):
    _, _, tf = route_solve(name, False)
    _, _, tp = route_solve(name, True)
    assert tf.size == tp.size and np.array_equal(tf.accepted, tp.accepted)
    print(name, "folded against separate pass: rel cost %.3e, rel radius %.3e" % (rel(tf.cost, tp.cost), rel(tf.radius, tp.radius)))
    assert rel(tf.cost, tp.cost) <= 1e-9 and rel(tf.radius, tp.radius) <= 1e-9


@pytest.mark.parametrize("name", list(CASES))
def test_two_runs_of_the_folded_route_are_bit_identical(name):
    again = gpu_solve(case_problem(name), case_options(name)[0], False)
    assert same_bits(route_solve(name, False), again)


def test_free_intrinsics_keep_the_separate_pass():
    """Outside the fold's condition the switch changes nothing: the same bits with it on and off."""
    p = synth.synth_ba_v1(12, 400, seed=0x5CA1E004, num_groups=4)
    o = ba.default_options()
    o.intrinsics_to_optimize = 0x01 | 0x10   # FOCAL_LENGTH | RADIAL_DISTORTION
    o.max_num_iterations = 6
    assert same_bits(gpu_solve(p, o, False), gpu_solve(p, o, True))
