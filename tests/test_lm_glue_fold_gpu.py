"""GPU: the folded chain of glue launches of an LM iteration (ba_solver.hip: lm_glue_applies) against the
separate launches it replaces, bit for bit.

Every case solves the same problem twice in one process: once with THEIA_HIP_LM_GLUE_KERNELS=1 (k_sp_clear, the
linearisation's k_reduce_tiles_stage1, k_finalize_rcs and k_sp_symm in launches of their own, every body) and once without
it (k_schur_sum adds the LM diagonal, the gradient maximum and the mirrored entries and carries the stage-1 sums;
k_cam_update finishes the linearisation's scalars and clears the reduced system; k_reduce_control clears the scalars and, on
an accepted step, flips LmState::cur instead of the copy of k_lm_accept -- the caps of 1, 2 and 7 end with the state in the
second, first and second buffers, so download, the second run, snapshot and restore see the host's pointer swap).
Nothing in the fold reorders a floating-point sum, so NO tolerance is used: the downloaded cameras and points, both costs,
the five trace arrays, num_iterations and termination_type must be equal bytes, after each step of

    run, download, run again on the same handle, snapshot, run, restore, run.

theia_hip_ba_lm_chain reports which chain a handle's run() takes (the value run() itself branches on): the cases the
predicate must send down the separate launches (inner iterations, free intrinsics) assert that it does, and are compared
with the switch on and off all the same.  The predicate needs a handle (its K3 plan and fused plan live on the device), so
it is tested here and not in a CPU file.

Scenes: synth_ba_v1 rings of 40 views (n = 240: four 64-wide tiles, so a camera's six columns straddle tile boundaries and
the K3 plan is sparse with three levels), 1500 tracks (about 9 000 observations: at most 9 000 / 54 = 167 wave tiles, the
single-stage reduction) and 6000 tracks (about 36 000 observations: more than 512 wave tiles, two stages).  The start
perturbations (multiples of synth_ba_v1's defaults) were chosen on the CPU oracle, whose accepted flags the cases assert:
  x16, seed 1, tolerances at zero: every step up to a cap of 1, 2 or 7 accepted (6000 tracks; with 1500 tracks the seventh
    is a cost change of 5e-13 relative, and only the first six are asserted);
  x30, seed 4: accepted 1 0 0 0 0 0 1 1 0 1 1 1 1 (rejections between accepted steps);
  x4, seed 1: stops by the function tolerance at iteration 4 (of 8 enqueued bodies, 4 run after done).
"""
import os

import numpy as np
import pytest

from pytheiasfm_amd import ba, synth

pytestmark = pytest.mark.gpu

SWITCH = "THEIA_HIP_LM_GLUE_KERNELS"


def scene(ntracks, scale, seed, const=False):
    p = synth.synth_ba_v1(40, ntracks, seed=seed, num_groups=3, sigma_pos=0.05 * scale, sigma_rot_deg=0.5 * scale, sigma_pt=0.02 * scale)
    if const:      # constant, position-only, orientation-only cameras (as tests/lm_rule_cases.py: main-constant-blocks); every fourth point
        cc = np.zeros(40, np.uint8); cc[[0, 6, 17, 31]] = 3; cc[[2, 20]] = 1; cc[[3, 33]] = 2; cc[10] = 4
        p.cam_const = cc
        pc = np.zeros(ntracks, np.uint8); pc[::4] = 1
        p.point_const = pc
    return p


FREE = dict(function_tolerance=0.0, gradient_tolerance=0.0, parameter_tolerance=0.0)      # only the cap ends the run


def options(max_it, **kw):
    o = ba.default_options()
    o.use_inner_iterations = 0
    o.max_num_iterations = max_it
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def record(h, s, tr):
    q = h.download(h.problem.copy())
    return dict(cam=q.cam_ext.copy(), pts=q.points.copy(), intr=q.intrinsics.copy(), initial=float(s.initial_cost), final=float(s.final_cost),
                its=int(s.num_iterations), term=int(s.termination_type), ok=int(s.success), cost=tr.cost.copy(),
                grad=tr.gradient_max_norm.copy(), step=tr.step_norm.copy(), radius=tr.radius.copy(), accepted=tr.accepted.copy())


def sequence(p, o, separate, env=None):
    """run, download, run, snapshot, run, restore, run on one handle; the record of each run, whether the chain was folded, K3 levels"""
    env = dict(env or {})
    if separate:
        env[SWITCH] = "1"
    old = {k: os.environ.get(k) for k in list(env) + [SWITCH]}
    os.environ.pop(SWITCH, None)
    os.environ.update(env)
    try:
        out = []
        with ba.BaHandle(p.copy(), o) as h:
            folded = h.lm_chain_folded()
            levels = h.plan_info()["k3_levels"]
            out.append(record(h, *h.run()))
            out.append(record(h, *h.run()))
            h.snapshot()
            out.append(record(h, *h.run()))
            h.restore()
            out.append(record(h, *h.run()))
            assert h.lm_chain_folded() == folded
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return out, folded, levels


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def compare(tag, p, o, want_folded=True, env=None):
    ref, f0, _ = sequence(p, o, True, env)
    new, f1, levels = sequence(p, o, False, env)
    assert not f0, "%s: the switch does not keep the separate launches" % tag
    assert f1 == want_folded, "%s: run() takes the %s chain" % (tag, "folded" if f1 else "separate")
    for k, (a, b) in enumerate(zip(ref, new)):
        print(tag, "run", k, "iterations", b["its"], "term", b["term"], "accepted", b["accepted"].tolist(), "cost %.17g -> %.17g" % (b["initial"], b["final"]))
        for key in a:
            x, y = a[key], b[key]
            eq = same_bytes(x, y) if isinstance(x, np.ndarray) else (np.float64(x).tobytes() == np.float64(y).tobytes() if isinstance(x, float) else x == y)
            assert eq, "%s: run %d: '%s' differs between the separate launches and the folded chain" % (tag, k, key)
    return new, levels


@pytest.mark.parametrize("scale_pass", [False, True], ids=["fold-first", "scale-pass"])
@pytest.mark.parametrize("max_it", [1, 2, 7])
def test_every_step_accepted_single_stage(max_it, scale_pass):
    p = scene(1500, 16.0, 1)
    assert p.obs_uv.shape[0] / 54.0 <= 512      # single-stage tile reduction (a wave tile holds 54 observations at least)
    new, levels = compare("accepted-%d%s" % (max_it, " scale-pass" if scale_pass else ""), p, options(max_it, **FREE), env={"THEIA_HIP_SCALE_PASS": "1"} if scale_pass else None)
    assert levels >= 3, levels
    # (the oracle accepts the seventh step of this scene too, but on a cost change of 5e-13 relative: not asserted here --
    # test_two_stage_reduction has seven steps that are accepted beyond doubt)
    assert new[0]["its"] == max_it and new[0]["accepted"].size == max_it + 1 and new[0]["accepted"][: min(max_it, 6) + 1].all()


@pytest.mark.parametrize("scale_pass", [False, True], ids=["fold-first", "scale-pass"])
def test_two_stage_reduction(scale_pass):
    p = scene(6000, 16.0, 1)
    assert p.obs_uv.shape[0] > 64 * 512         # more than 512 wave tiles: two stages
    new, levels = compare("two-stage%s" % (" scale-pass" if scale_pass else ""), p, options(7, **FREE), env={"THEIA_HIP_SCALE_PASS": "1"} if scale_pass else None)
    assert levels >= 3, levels
    assert new[0]["its"] == 7 and new[0]["accepted"].all()


def test_rejected_steps_between_accepted_ones():
    new, _ = compare("rejected", scene(1500, 30.0, 4), options(12))
    acc = new[0]["accepted"].tolist()
    assert acc == [1, 0, 0, 0, 0, 0, 1, 1, 0, 1, 1, 1, 1], acc      # (the oracle's flags)


def test_tolerance_stop_with_bodies_after_done():
    new, _ = compare("tolerance-stop", scene(1500, 4.0, 1), options(8))
    assert new[0]["term"] == 0 and new[0]["its"] == 4, (new[0]["term"], new[0]["its"])      # CONVERGENCE before the cap of 8 (one chunk of 8 bodies)


@pytest.mark.parametrize("ntracks", [1500, 6000])
def test_constant_cameras_and_points(ntracks):
    new, _ = compare("constant-blocks-%d" % ntracks, scene(ntracks, 16.0, 3, const=True), options(7))
    assert new[0]["its"] >= 2


def test_inner_iterations_keep_the_separate_launches():
    compare("inner", scene(1500, 16.0, 1), options(4, use_inner_iterations=1), want_folded=False)


def test_free_intrinsics_keep_the_separate_launches():
    compare("intrinsics", scene(1500, 4.0, 1), options(4, intrinsics_to_optimize=0x11), want_folded=False)


def test_phase_timing_keeps_the_separate_launches():
    compare("phase-timing", scene(1500, 16.0, 1), options(3), want_folded=False, env={"THEIA_HIP_PHASE_TIMING": "1"})
