"""GPU: every template instance of the BA hot path (loss class x camera-model set x point parametrisation x compound block
width) against the CPU oracle, on the edge scenes of tests/ba_edge_scenes.py.

Every case compares the start state with the oracle (cost, residuals, Jacobians, the reduced system at radius 1e4) and then
a solve of max_num_iterations = 2 in a FRESH handle: the trace's cost, radius, step_norm and gradient_max_norm go through the
back-substitution and the candidate evaluation of the instance.  A pytest item is one (route, camera model); it loops over
loss x PD (x intrinsics mask), prints the figures of every case and collects the failures, so that one bad instance names
itself and does not hide the rest.

Bounds (relative, max norm), each from the test it is the project's bound in:
  cost 1e-12, residuals and Jacobians 1e-11 (test_ba_gpu.test_robust_losses_match_oracle), intrinsics Jacobian 1e-10 per
  column (test_intrinsics_jacobian_matches_jet_oracle), S and rhs 1e-10, 1e-9 with free intrinsics
  (test_reduced_camera_system_matches_oracle, test_intrinsics_jacobian_matches_jet_oracle); accepted flags equal, trace cost
  and radius 1e-9, step_norm 1e-6, gradient_max_norm 1e-6 of its largest entry (test_scale_fold_gpu), intrinsics after the
  solve 1e-7 (test_intrinsics_optimisation_lm_parity_and_recovery).

Where the reference itself is less certain than a bound, the bound comes from the reference: oracle_noise() solves the case
again from an input perturbed by 1e-15 relative and the case carries ten times the largest deviation of the oracle from
itself (the factor is for the order of summation); both numbers are printed with the case.  Measured on an MI355X, worst
over the cases of a class, device against oracle | oracle against itself:
  PD 3, every route, all models but the orthographic: cost 2e-11, radius 3e-11, step 2e-10, gradient 8e-11 | below a tenth
    of the bounds (the project's bounds hold);
  orthographic model (the depth of every camera is a gauge direction), PD 3: step 4e-11 | 1.7e-6; PD 4: step 6e-7 | 9e-5;
  PD 4 on the edge scene: cost 1.2e-4, step 2.9e-2 (1.4e-2 with long tracks) | cost 8.5e-2, step 4.8.  The ambient
    parametrisation is singular at two of the plants: the homogeneous scale of the point at the origin is the w axis, whose
    Jacobian column is pure round-off, and the block is invertible only through the LM floor; the on-axis points behave
    alike.  The Householder branch the origin stands for does not exist with PD 4.  So every PD 4 case runs its solve a second
    time on es.off_the_edges (origin and on-axis points moved by 1e-3): cost 2.9e-9, radius 7.8e-9, step 3.4e-8, gradient
    8e-9 | cost 8.9e-9, radius 3.5e-8; the start-state comparisons (Jacobians 1e-11, S and rhs 1e-10) are on the edge
    scene for both parametrisations and need no allowance;
  inner iterations with free intrinsics (a rejected candidate's swept cost): cost 1.0e-1, step 1.1e-3 | cost 1.6e-1, 5e-3;
  FOV with a free omega of 5e-4 (both steps are wild and rejected, costs of 3e11): the closest case of the module,
    intr_gather model=3 trivial pd=4 0x11 off the edges, cost 2.87e-9 against its bound of 3.7e-9.
No case's figure is above 0.25 of its bound except that one (0.78).

The matrix found one defect, fixed with it: a solve that stopped at the iteration cap right after an accepted step reported
-1 as that step's gradient_max_norm (every case here does: max_num_iterations = 2).

Which instance a handle dispatches to is read from theia_hip_ba_kernel_instances, whose values come from the host helpers
the launch sites branch on.  Every case records the strings of its handles; the last test of the module asserts that their
union is the full list the dispatch can produce, written out there.

Block width of the fused intrinsics path (ba_plan.hip, classify_blocks): the largest number of free parameters of a group
gives 9 for up to three, 10 for four, 13 for five to seven, 16 for eight to ten; width 9 with the free set {focal, the two
radial parameters 5 and 6} in every free group is the FOCAL_LENGTH | RADIAL_DISTORTION instance (kmask=1).  INTR_MASKS maps
each model's option masks to their parameter count."""
import functools
import os

import numpy as np
import pytest

from pytheiasfm_amd import _capi as capi, ba
from tests import ba_edge_scenes as es
from tests import oracle_lib as ol

pytestmark = pytest.mark.gpu

RAN = set()         # the instance strings of every handle the module ran
ROUTES = set()      # the routes that ran (the union test needs all of them)
ALL_ROUTES = {"main", "intr", "schur_gather", "intr_gather", "long", "inner"}

# THEIA_INTR_*: FOCAL 0x01, ASPECT 0x02, SKEW 0x04, PRINCIPAL_POINTS 0x08, RADIAL 0x10, TANGENTIAL 0x20.
# model: [(mask, free parameters per group, block width, kmask)]
INTR_MASKS = {
    0: [(0x11, 3, 9, 1), (0x07, 3, 9, 0), (0x13, 4, 10, 0), (0x3f, 7, 13, 0)],          # pinhole: f + k1 k2 | f a s | f a k1 k2 | all 7
    1: [(0x11, 4, 10, 0), (0x3f, 10, 16, 0)],                                          # radial-tangential: f + k1 k2 k3 | all 10
    2: [(0x07, 3, 9, 0), (0x10, 4, 10, 0), (0x11, 5, 13, 0), (0x3f, 9, 16, 0)],          # fisheye: f a s | k1..k4 | f + k1..k4 | all 9
    3: [(0x11, 2, 9, 0), (0x0b, 4, 10, 0), (0x3f, 5, 13, 0)],                            # FOV: f omega | f a cx cy | all 5
    5: [(0x11, 3, 9, 1), (0x3f, 7, 13, 0)],                                            # double sphere: f xi alpha | all 7
    "mixed": [(0x11, 3, 9, 1)],                                                        # pinhole + double sphere free, FOV group constant
}
INTR_LOSSES = (0, 1, 4)     # trivial, Huber, Arctan


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(b).max(), 1e-300)) if np.size(b) else 0.0


@functools.lru_cache(maxsize=None)
def scene(kind, model, loss):
    perturb = 1.0 if loss == 0 else es.ROBUST_PERTURB
    if model == "mixed":
        p = es.mixed_scene(perturb=perturb)
    else:
        p = es.edge_scene(model, perturb=perturb)
    if kind.endswith("+off"):
        p = es.off_the_edges(p)
    if kind.startswith("long"):
        p = es.with_long_tracks(p)
    if kind.startswith("priors"):
        p = es.with_position_priors(p)
    return p


def options(side, loss, pd, intr=0, inner=0, priors=0, iters=2):
    o = ba.default_options() if side == "gpu" else ol.default_options()
    return es.set_case(o, loss, pd, intrinsics_to_optimize=intr, use_inner_iterations=inner, prior_mask=priors, max_num_iterations=iters)


@functools.lru_cache(maxsize=None)
def oracle_case(kind, model, loss, pd, intr, inner, priors):
    """The oracle's side of a case, computed once and shared by the routes that run it."""
    p = scene(kind, model, loss)
    oo = options("oracle", loss, pd, intr, inner, priors)
    ev = ol.evaluate_ex(p, oo) if intr else ol.evaluate(p, oo) + (None,)
    S, rhs = ol.reduced_system(p, oo, 1e4)
    po = p.copy()
    so, tro = ol.solve(po, oo)
    return ev, S, rhs, po, so, tro


# the project's bounds on the trace (see the module docstring); a case whose reference is itself less certain than that
# carries 10 x the reference's own deviation instead (the factor is for the order of summation)
TRACE_BOUNDS = {"cost": 1e-9, "radius": 1e-9, "step": 1e-6, "gradient": 1e-6, "intrinsics": 1e-7}
NOISE_DRAWS = (3, 12)     # three draws; twelve where the first three show the reference less certain than a tenth of a bound


@functools.lru_cache(maxsize=None)
def oracle_noise(kind, model, loss, pd, intr, inner, priors):
    """The oracle against itself: the same solve with its input (extrinsics, points, intrinsics, observations) perturbed
    by 1e-15 relative, the largest deviation of each trace quantity over the draws.  This is the reference's own error on
    the case; `stable` says whether its accepted flags and failed candidates survived the perturbation at all."""
    p = scene(kind, model, loss)
    oo = options("oracle", loss, pd, intr, inner, priors)
    _, _, _, po, so, tro = oracle_case(kind, model, loss, pd, intr, inner, priors)
    fin = tro.cost < 1e300
    out = {"cost": 0.0, "radius": 0.0, "step": 0.0, "gradient": 0.0, "intrinsics": 0.0, "stable": True}
    for draw in range(NOISE_DRAWS[1]):
        if draw == NOISE_DRAWS[0] and out["stable"] and all(out[k] <= 0.1 * b for k, b in TRACE_BOUNDS.items()):
            break
        rng = np.random.default_rng(0x5E5 + draw)
        q = p.copy()
        q.obs_uv = q.obs_uv * (1.0 + 1e-15 * rng.standard_normal(q.obs_uv.shape))
        q.cam_ext = q.cam_ext * (1.0 + 1e-15 * rng.standard_normal(q.cam_ext.shape))
        q.points = q.points * (1.0 + 1e-15 * rng.standard_normal(q.points.shape))
        q.intrinsics = q.intrinsics * (1.0 + 1e-15 * rng.standard_normal(q.intrinsics.shape))
        s, tr = ol.solve(q, oo)
        if tr.size != tro.size or not np.array_equal(tr.accepted, tro.accepted) or not np.array_equal(tr.cost < 1e300, fin):
            out["stable"] = False
            continue
        dev = {"cost": rel(tr.cost[fin], tro.cost[fin]), "radius": rel(tr.radius, tro.radius), "step": rel(tr.step_norm, tro.step_norm),
               "gradient": float(np.abs(tr.gradient_max_norm - tro.gradient_max_norm).max() / tro.gradient_max_norm.max()),
               "intrinsics": rel(q.intrinsics, po.intrinsics)}
        for k, v in dev.items():
            out[k] = max(out[k], v)
    return out




def gpu_solve(p, o, scale_pass=False):
    """One solve in a fresh handle (the first launch of a fresh handle takes the fold, unless the switch, which every run
    reads, forces the separate column-norm pass); returns the problem, summary, trace and the handle's instance strings."""
    old = os.environ.pop("THEIA_HIP_SCALE_PASS", None)
    if scale_pass:
        os.environ["THEIA_HIP_SCALE_PASS"] = "1"
    try:
        pg = p.copy()
        with ba.BaHandle(pg, o) as h:
            inst = h.kernel_instances()
            s, tr = h.run()
            h.download(pg)
    finally:
        os.environ.pop("THEIA_HIP_SCALE_PASS", None)
        if old is not None:
            os.environ["THEIA_HIP_SCALE_PASS"] = old
    return pg, s, tr, inst


def check(fails, tag, name, value, bound):
    if not value <= bound:
        fails.append("%s: %s %.3e > %.1e" % (tag, name, value, bound))


def compare_trace(fails, tag, got, want, intr, noise):
    pg, s, tr = got
    po, so, tro = want
    if not noise["stable"]:
        # the reference has no answer to compare with: its own accepted flags change when its input moves by 1e-15
        fails.append("%s: the oracle's own trajectory does not survive a 1e-15 perturbation of its input" % tag)
        return
    if tr.size != tro.size or not np.array_equal(tr.accepted, tro.accepted) or s.num_iterations != so.num_iterations:
        fails.append("%s: accepted %s against the oracle's %s" % (tag, tr.accepted.tolist(), tro.accepted.tolist()))
        print(tag, "accepted", tr.accepted.tolist(), "oracle", tro.accepted.tolist(), "cost", tr.cost.tolist(), "oracle", tro.cost.tolist())
        return
    fin = tro.cost < 1e300       # (a candidate that failed to evaluate is recorded as DBL_MAX on both sides)
    same_failed = bool(np.array_equal(fin, tr.cost < 1e300))
    fig = {"cost": rel(tr.cost[fin], tro.cost[fin]), "radius": rel(tr.radius, tro.radius), "step": rel(tr.step_norm, tro.step_norm),
           "gradient": float(np.abs(tr.gradient_max_norm - tro.gradient_max_norm).max() / tro.gradient_max_norm.max()),
           "cam": float(np.abs(pg.cam_ext - po.cam_ext).max()), "points": float(np.abs(pg.points - po.points).max()),
           "intrinsics": rel(pg.intrinsics, po.intrinsics) if intr else 0.0}
    bound = {k: max(b, 10.0 * noise[k]) for k, b in TRACE_BOUNDS.items()}
    print(tag, "accepted", tr.accepted.tolist(), " ".join("%s %.2e" % kv for kv in fig.items()),
          "| oracle's own", " ".join("%s %.1e" % (k, noise[k]) for k in TRACE_BOUNDS if noise[k] > 0.1 * TRACE_BOUNDS[k]),
          "| worst figure / bound %.2f" % max(fig[k] / bound[k] for k in TRACE_BOUNDS))
    if not same_failed:
        fails.append("%s: failed candidates %s against the oracle's %s" % (tag, (~(tr.cost < 1e300)).tolist(), (~fin).tolist()))
    if s.success != so.success or s.termination_type != so.termination_type:
        fails.append("%s: success / termination %d %d against %d %d" % (tag, s.success, s.termination_type, so.success, so.termination_type))
    check(fails, tag, "initial cost", abs(s.initial_cost - so.initial_cost) / so.initial_cost, 1e-12)
    check(fails, tag, "trace cost", fig["cost"], bound["cost"])
    check(fails, tag, "trace radius", fig["radius"], bound["radius"])
    check(fails, tag, "step_norm", fig["step"], bound["step"])
    check(fails, tag, "gradient_max_norm", fig["gradient"], bound["gradient"])
    if intr:
        check(fails, tag, "intrinsics", fig["intrinsics"], bound["intrinsics"])


def run_case(fails, route, kind, model, loss, pd, intr=0, inner=0, priors=0, scale_pass_too=False, plan=None, expect=()):
    """One case on the route the environment selects: start state, reduced system, two LM iterations, all against the oracle.
    plan: the (fused_runs, slow_path_tracks) test the handle must pass; expect: substrings one of the handle's instance
    strings must carry each."""
    tag = "%s model=%s %s pd=%d intr=0x%02x%s%s" % (route, model, es.LOSS_NAMES[loss], pd, intr, " inner" if inner else "", " priors" if priors else "")
    p = scene(kind, model, loss)
    o = options("gpu", loss, pd, intr, inner, priors)
    ev, So, rhso, po, so, tro = oracle_case(kind, model, loss, pd, intr, inner, priors)
    ok, ocost, orr, ojc, ojp, oji = ev
    with ba.BaHandle(p.copy(), o) as h:
        info = h.plan_info()
        inst = h.kernel_instances()
        if intr:
            cost, r, jc, jp, ji, valid = h.evaluate_ex()
        else:
            cost, r, jc, jp, valid = h.evaluate(); ji = None
        S, rhs = h.reduced_system(1e4)
    RAN.update(inst)
    if plan is not None and not plan(info):
        fails.append("%s: plan %s" % (tag, info))
    for want in expect:
        if not any(want in line for line in inst):
            fails.append("%s: no instance with '%s' in %s" % (tag, want, inst))
    fig = {"cost": abs(cost - ocost) / ocost, "r": rel(r, orr), "Jc": rel(jc, ojc), "Jp": rel(jp, ojp), "S": rel(S, So), "rhs": rel(rhs, rhso)}
    if intr:
        fig["Jk"] = max(float(np.abs(ji[:, :, q] - oji[:, :, q]).max() / max(np.abs(oji[:, :, q]).max(), 1e-300)) for q in range(10))
    print(tag, "runs %d slow %d" % (info["fused_runs"], info["slow_path_tracks"]), " ".join("%s %.2e" % kv for kv in fig.items()))
    if ok != 1 or not valid.all():
        fails.append("%s: invalid observations at the start (oracle ok %d, device %d invalid)" % (tag, ok, int((valid == 0).sum())))
    if S.shape != So.shape:
        fails.append("%s: reduced system %s against %s" % (tag, S.shape, So.shape))
    check(fails, tag, "cost", fig["cost"], 1e-12)
    check(fails, tag, "residuals", fig["r"], 1e-11)
    check(fails, tag, "camera Jacobian", fig["Jc"], 1e-11)
    check(fails, tag, "point Jacobian", fig["Jp"], 1e-11)
    if intr:
        check(fails, tag, "intrinsics Jacobian", fig["Jk"], 1e-10)
    check(fails, tag, "S", fig["S"], 1e-9 if intr else 1e-10)
    check(fails, tag, "rhs", fig["rhs"], 1e-9 if intr else 1e-10)
    noise = oracle_noise(kind, model, loss, pd, intr, inner, priors)
    pg, s, tr, inst2 = gpu_solve(p, o)
    RAN.update(inst2)
    compare_trace(fails, tag, (pg, s, tr), (po, so, tro), intr, noise)
    if scale_pass_too:
        pg, s, tr, inst3 = gpu_solve(p, o, scale_pass=True)
        RAN.update(inst3)
        if any("first=1" in line for line in inst3) or not any("first=1" in line for line in inst2):
            fails.append("%s: the fold switch does not select the first-launch instance: %s / %s" % (tag, inst2, inst3))
        compare_trace(fails, tag + " [separate scale pass]", (pg, s, tr), (po, so, tro), intr, noise)
    if pd == 4:
        # the ambient parametrisation once more on the scene without the two plants that make its point blocks singular
        # (es.off_the_edges): there the reference is certain and the project's bounds hold
        kind2 = kind + "+off"
        _, _, _, po, so, tro = oracle_case(kind2, model, loss, pd, intr, inner, priors)
        pg, s, tr, inst4 = gpu_solve(scene(kind2, model, loss), o)
        RAN.update(inst4)
        compare_trace(fails, tag + " [off the edges]", (pg, s, tr), (po, so, tro), intr, oracle_noise(kind2, model, loss, pd, intr, inner, priors))


def fused(info):
    return info["fused_runs"] >= 2 and info["slow_path_tracks"] == 0


def lossk3(loss):
    return 0 if loss == 0 else (2 if loss in (3, 4) else 1)


def models_of(model):
    return "all" if model in (2, 3, "mixed") else "notrig"


# ---------------------------------------------------------------- the routes
@pytest.mark.parametrize("model", range(8))
def test_main_fused_path(model):
    """k_lin_schur (with and without the first-launch fold) and k_backsub_runs: 8 models x 7 losses x PD {3, 4}."""
    fails = []
    for loss in es.LOSSES:
        for pd in (3, 4):
            want = "pd=%d models=%s lossk=%d" % (pd, models_of(model), lossk3(loss))
            run_case(fails, "main", "edge", model, loss, pd, scale_pass_too=True, plan=fused,
                     expect=("k_lin_schur " + want + " first=0", "k_backsub_runs " + want))
    ROUTES.add("main")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("model", list(INTR_MASKS))
def test_fused_intrinsics_path(model):
    """k_lin_schur_i and the intrinsics k_backsub_runs: every block width and the FOCAL | RADIAL instance."""
    fails = []
    for mask, _, bw, kmask in INTR_MASKS[model]:
        for loss in INTR_LOSSES:
            for pd in (3, 4):
                want = "pd=%d models=%s lossk=%d" % (pd, models_of(model), 0 if loss == 0 else 2)
                run_case(fails, "intr", "edge", model, loss, pd, intr=mask, plan=fused,
                         expect=("k_lin_schur_i %s bw=%d kmask=%d" % (want, bw, kmask), "k_backsub_runs %s waves=2 intr=1 kmask=%d" % (want, kmask)))
    ROUTES.add("intr")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("model", range(8))
def test_schur_gather_kernels(model, monkeypatch):
    """The same cases on the gather kernels (k_lin_obs + k_schur, k_backsub): the switch is read when the handle is made."""
    monkeypatch.setenv("THEIA_HIP_SCHUR_GATHER", "1")
    fails = []
    for loss in es.LOSSES:
        for pd in (3, 4):
            run_case(fails, "schur_gather", "edge", model, loss, pd, plan=lambda info: info["fused_runs"] == 0,
                     expect=("k_lin_obs pd=%d" % pd, "k_backsub pd=%d intr=0 rot=0" % pd))
    ROUTES.add("schur_gather")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("model", list(INTR_MASKS))
def test_intrinsics_gather_kernels(model, monkeypatch):
    """The free-intrinsics cases on the gather lists (k_lin_obs_intr + k_schur_intr, k_backsub with intrinsics)."""
    monkeypatch.setenv("THEIA_HIP_INTR_GATHER", "1")
    fails = []
    for mask, nfree, _, _ in INTR_MASKS[model]:
        for loss in INTR_LOSSES:
            for pd in (3, 4):
                run_case(fails, "intr_gather", "edge", model, loss, pd, intr=mask, plan=lambda info: info["fused_runs"] == 0,
                         expect=("k_lin_obs_intr pd=%d ki=%d" % (pd, 4 if nfree <= 4 else 10), "k_backsub pd=%d intr=1 rot=0" % pd))
    ROUTES.add("intr_gather")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("model", range(8))
def test_long_track_path(model):
    """The edge scene plus two tracks of 65 observations (more than a wave tile holds): the per-observation kernels beside
    the fused ones, without and with free intrinsics."""
    fails = []
    for loss in INTR_LOSSES:
        for pd in (3, 4):
            for intr in (0, 0x11):
                run_case(fails, "long", "long", model, loss, pd, intr=intr, plan=lambda info: info["slow_path_tracks"] == 2 and info["fused_runs"] >= 2,
                         expect=("k_long pd=%d intr=%d" % (pd, 1 if intr else 0),))
    ROUTES.add("long")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("model", [0, 3, 5])
def test_inner_iterations(model):
    """use_inner_iterations = 1: the lean instances of k_inner_views / k_inner_groups with loss class 0 and 1, their
    <kModelsAll, 2> instances (FOV, or Cauchy), both group row counts, and every k_inner_tracks instance; with camera priors
    the views instance that carries them."""
    fails = []
    for loss in (0, 1, 3):
        lean = model != 3 and loss != 3
        vg = "models=%s lossk=%d" % ("notrig" if lean else "all", (0 if loss == 0 else 1) if lean else 2)
        for pd in (3, 4):
            trk = "k_inner_tracks pd=%d models=%s lossk=%d" % (pd, models_of(model), lossk3(loss))
            run_case(fails, "inner", "edge", model, loss, pd, inner=1, plan=fused, expect=("k_inner_views %s priors=0" % vg, trk))
            run_case(fails, "inner", "edge", model, loss, pd, intr=0x11, inner=1, plan=fused, expect=("k_inner_groups %s kc=4" % vg, trk))
            run_case(fails, "inner", "edge", model, loss, pd, intr=0x3f, inner=1, plan=fused, expect=("k_inner_groups %s kc=10" % vg, trk))
        run_case(fails, "inner", "priors", model, loss, 3, inner=1, priors=1, expect=("k_inner_views %s priors=1" % vg,))
    ROUTES.add("inner")
    assert not fails, "\n".join(fails)


# ---------------------------------------------------------------- the batch kernels
@pytest.mark.parametrize("model", [3, 4, 6, 7])
def test_views_batch_on_camera_slices(model):
    """theia_hip_ba_views_batch on the scene cut into one localisation problem per camera, for the models the batch tests
    do not reach (FOV, division undistortion, extended unified, orthographic); trivial and Huber loss.  Bounds: those of
    test_ba_gpu.test_views_batch_matches_per_problem_oracle."""
    fails = []
    p = es.edge_scene(model)
    offs, uv, X, cams, intr, mods, flats = es.camera_slices(p)
    for loss in (0, 1):
        o = options("gpu", loss, 4, iters=15)
        oo = options("oracle", loss, 4, iters=15)
        cam_gpu = cams.copy()
        summ = ba.solve_views_batch(offs, uv, X, cam_gpu, intr, mods, o)
        for c, fp in enumerate(flats):
            fo = fp.copy()
            so, _ = ol.solve(fo, oo)
            s = summ[c]
            tag = "views model=%d %s camera %d" % (model, es.LOSS_NAMES[loss], c)
            fig = (abs(s.initial_cost - so.initial_cost) / so.initial_cost, abs(s.final_cost - so.final_cost) / so.final_cost,
                   float(np.abs(cam_gpu[c] - fo.cam_ext[0]).max()))
            print(tag, "iterations %d / %d" % (s.num_iterations, so.num_iterations), "initial %.2e final %.2e cam %.2e" % fig)
            if (s.success, s.termination_type, s.num_iterations, s.num_successful_steps) != (so.success, so.termination_type, so.num_iterations, so.num_successful_steps):
                fails.append("%s: summary (%d %d %d %d) against (%d %d %d %d)" % (tag, s.success, s.termination_type, s.num_iterations, s.num_successful_steps,
                                                                                so.success, so.termination_type, so.num_iterations, so.num_successful_steps))
                continue
            check(fails, tag, "initial cost", fig[0], 1e-10)
            check(fails, tag, "final cost", fig[1], 1e-9)
            check(fails, tag, "camera", fig[2], 1e-9)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("model", [3, 4, 6, 7])
def test_tracks_batch_on_track_slices(model):
    """theia_hip_ba_tracks_batch on the scene (every point on its own, cameras constant) for the same four models, both
    point parametrisations: the planted points and every sixth of the others against the per-track oracle.  Bounds: those
    of test_ba_gpu.test_tracks_batch_matches_per_track_oracle, or ten times the oracle's own deviation on the track
    where that is larger (orthographic tracks in the ambient parametrisation: X - w C does not change along (C, 1)).
    PD 4 runs on es.off_the_edges: a point at the origin has no reference there -- its w column is round-off, and the
    device's point differed from the oracle's by 2.6e-3 where the oracle's own moved by 5.4e-5 under 1e-15 perturbations,
    neither of them a number that means anything."""
    fails = []
    tracks = sorted(set(range(25)) | set(range(25, es.edge_scene(model).points.shape[0], 6)))
    for pd in (3, 4):
        p = es.edge_scene(model) if pd == 3 else es.off_the_edges(es.edge_scene(model))
        o = options("gpu", 0, pd, iters=20)
        oo = options("oracle", 0, pd, iters=20)
        pg = p.copy()
        summ = ba.solve_tracks_batch(pg, o)
        unstable = []
        worst = [0.0, 0.0, 0.0]
        for t in tracks:
            fp = es.track_slice(p, t)
            so, _ = ol.solve(fp, oo)
            s = summ[t]
            tag = "tracks model=%d pd=%d track %d" % (model, pd, t)
            # the reference's own error on this track: its input moved by 1e-15 relative
            noise, same = [0.0, 0.0], True
            for draw in range(3):
                rng = np.random.default_rng(1000 * draw + t)
                fq = es.track_slice(p, t)
                fq.points = fq.points * (1.0 + 1e-15 * rng.standard_normal(fq.points.shape))
                fq.cam_ext = fq.cam_ext * (1.0 + 1e-15 * rng.standard_normal(fq.cam_ext.shape))
                fq.obs_uv = fq.obs_uv * (1.0 + 1e-15 * rng.standard_normal(fq.obs_uv.shape))
                sq, _ = ol.solve(fq, oo)
                same = same and (sq.success, sq.num_iterations, sq.num_successful_steps) == (so.success, so.num_iterations, so.num_successful_steps)
                noise = [max(noise[0], abs(sq.final_cost - so.final_cost) / max(so.final_cost, 1e-300)), max(noise[1], float(np.abs(fq.points[0] - fp.points[0]).max()))]
            if not same:
                unstable.append(t)     # (no answer to compare with: the oracle's own iteration count changes)
                continue
            if (s.success, s.num_iterations, s.num_successful_steps) != (so.success, so.num_iterations, so.num_successful_steps):
                fails.append("%s: summary (%d %d %d) against (%d %d %d)" % (tag, s.success, s.num_iterations, s.num_successful_steps,
                                                                          so.success, so.num_iterations, so.num_successful_steps))
                continue
            fig = (abs(s.initial_cost - so.initial_cost) / max(so.initial_cost, 1e-300), abs(s.final_cost - so.final_cost) / max(so.final_cost, 1e-300),
                   float(np.abs(pg.points[t] - fp.points[0]).max()))
            worst = [max(a, b) for a, b in zip(worst, fig)]
            check(fails, tag, "initial cost", fig[0], 1e-10)
            if max(noise) > 1e-10:
                print(tag, "final %.2e point %.2e | oracle's own %.1e %.1e" % (fig[1], fig[2], noise[0], noise[1]))
            check(fails, tag, "final cost", fig[1], max(1e-9, 10.0 * noise[0]))
            check(fails, tag, "point", fig[2], max(1e-9, 10.0 * noise[1]))
        print("tracks model=%d pd=%d: %d tracks, worst initial %.2e final %.2e point %.2e; oracle unstable on %s" % ((model, pd, len(tracks)) + tuple(worst) + (unstable,)))
        if unstable:
            fails.append("tracks model=%d pd=%d: the oracle's own iteration count changes under a 1e-15 perturbation on tracks %s" % (model, pd, unstable))
    assert not fails, "\n".join(fails)


# ---------------------------------------------------------------- invalid observations through the hot path
@pytest.mark.parametrize("intr", [0, 0x11])
def test_observation_invalid_at_the_start(intr):
    """A double-sphere scene whose start state has one point (w = -1) in the model's invalid region: the solve fails as
    the oracle's does, at once, and returns the parameters untouched."""
    p = es.invalid_start_scene()
    for pd in (3, 4):
        o, oo = options("gpu", 0, pd, intr, iters=5), options("oracle", 0, pd, intr, iters=5)
        with ba.BaHandle(p.copy(), o) as h:
            valid = h.evaluate()[4]
        print("invalid at the start: pd", pd, "intr", intr, "device invalid", int((valid == 0).sum()))
        assert (valid == 0).sum() == es.branch_counts(p)["invalid"] >= 1
        pg, s, tr, inst = gpu_solve(p, o)
        RAN.update(inst)
        po = p.copy()
        so, tro = ol.solve(po, oo)
        assert (s.success, s.termination_type, s.num_iterations) == (so.success, so.termination_type, so.num_iterations) == (0, so.termination_type, 0)
        assert np.array_equal(pg.cam_ext, p.cam_ext) and np.array_equal(pg.points, p.points) and np.array_equal(pg.intrinsics, p.intrinsics)


@pytest.mark.parametrize("intr", [0, 0x11])
@pytest.mark.parametrize("pd", [3, 4])
def test_observation_invalid_only_at_a_candidate(pd, intr):
    """The scene of es.invalid_candidate_scene(): valid at the start, the first candidates invalid in one camera.  The
    device must reject and accept the steps the oracle does, with its radii (test_ba_edge_scenes asserts, with the
    oracle alone, that the first step is rejected because it fails to evaluate)."""
    p, _, _ = es.invalid_candidate_scene()
    o, oo = options("gpu", 0, pd, intr, iters=8), options("oracle", 0, pd, intr, iters=8)
    pg, s, tr, inst = gpu_solve(p, o)
    RAN.update(inst)
    po = p.copy()
    so, tro = ol.solve(po, oo)
    print("invalid candidate: pd", pd, "intr", intr, "accepted", tr.accepted.tolist(), "oracle", tro.accepted.tolist(),
          "rel radius %.2e" % (rel(tr.radius, tro.radius) if tr.size == tro.size else np.inf))
    assert tro.accepted[1] == 0 and tro.cost[1] > 1e300
    assert tr.size == tro.size and np.array_equal(tr.accepted, tro.accepted)
    assert np.array_equal(tr.cost > 1e300, tro.cost > 1e300)
    assert rel(tr.radius, tro.radius) <= 1e-9
    fin = tro.cost < 1e300
    assert rel(tr.cost[fin], tro.cost[fin]) <= 1e-9


# ---------------------------------------------------------------- which instances ran
def expected_instances():
    """Every instance string the dispatch can produce for the kernel families of this module, written out."""
    out = set()
    for pd in (3, 4):
        for models in ("notrig", "all"):
            for lossk in (0, 1, 2):
                for first in (0, 1):
                    out.add("k_lin_schur pd=%d models=%s lossk=%d first=%d" % (pd, models, lossk, first))
                out.add("k_inner_tracks pd=%d models=%s lossk=%d" % (pd, models, lossk))
            for lossk, waves in ((0, 3), (0, 2), (1, 2), (2, 2)):
                out.add("k_backsub_runs pd=%d models=%s lossk=%d waves=%d intr=0 kmask=0" % (pd, models, lossk, waves))
            for lossk in (0, 2):
                for bw, kmask in ((9, 1), (9, 0), (10, 0), (13, 0), (16, 0)):
                    out.add("k_lin_schur_i pd=%d models=%s lossk=%d bw=%d kmask=%d" % (pd, models, lossk, bw, kmask))
                for kmask in (0, 1):
                    out.add("k_backsub_runs pd=%d models=%s lossk=%d waves=2 intr=1 kmask=%d" % (pd, models, lossk, kmask))
        out.add("k_lin_obs pd=%d" % pd)
        for ki in (4, 10):
            out.add("k_lin_obs_intr pd=%d ki=%d" % (pd, ki))
        for intr in (0, 1):
            out.add("k_backsub pd=%d intr=%d rot=0" % (pd, intr))
            out.add("k_long pd=%d intr=%d" % (pd, intr))
    for models, lossk in (("notrig", 0), ("notrig", 1), ("all", 2)):
        for priors in (0, 1):
            out.add("k_inner_views models=%s lossk=%d priors=%d" % (models, lossk, priors))
        for kc in (4, 10):
            out.add("k_inner_groups models=%s lossk=%d kc=%d" % (models, lossk, kc))
    return out


# Not reachable in this process: k_backsub_runs<PD, 4, MODELS, 0, 2> (trivial loss at two waves per SIMD) is taken only when
# THEIA_HIP_BACKSUB_WAVES is set to something other than 3, and the launch site reads that switch once per process.
EXCLUDED = {"k_backsub_runs pd=%d models=%s lossk=0 waves=2 intr=0 kmask=0" % (pd, models) for pd in (3, 4) for models in ("notrig", "all")}


def test_every_dispatchable_instance_ran():
    """The union of the instance strings of the cases above is the full list, less the excluded instance."""
    if ROUTES != ALL_ROUTES:
        pytest.skip("needs every route of this module in the same process (ran: %s)" % sorted(ROUTES))
    want = expected_instances()
    assert len(want) == 24 + 12 + 16 + 40 + 16 + 2 + 4 + 4 + 4 + 6 + 6 and EXCLUDED < want
    print("%d instance strings ran, %d expected, %d excluded" % (len(RAN), len(want), len(EXCLUDED)))
    for line in sorted(RAN):
        print("  ", line)
    assert RAN == want - EXCLUDED, "never ran: %s; not in the list: %s" % (sorted(want - EXCLUDED - RAN), sorted(RAN - want))
