"""Cases and the bracketing helper that pin the three tolerance rules of every LM loop -- TEST SIDE ONLY, no GPU.

Every loop of the library (and its counterpart in the oracle) ends a solve by one of

    function    |cost change| <= function_tolerance * cost                       (candidate step, before accept / reject)
    gradient    max |gradient| <= gradient_tolerance                             (after successful steps only)
    parameter   |step| <= parameter_tolerance * (|x| + parameter_tolerance)      (candidate step, before accept / reject)

At the default tolerances the function rule ends nearly every run, so nothing is decided on the values the other two read
(|x| of the variable blocks above all).  The bundle-adjustment trajectories converge quadratically: the quantity of each rule
falls by a factor of ten or more per iteration, so a tolerance can be placed sharply between two iterations.
critical_tolerance() bisects, on the ORACLE, the tolerance t* at which a run with the other two tolerances at zero changes from
stopping at iteration <= stop_at to stopping later, and returns the bracket (t* (1 + w), t* (1 - w)); the device must stop where
its oracle stops at both values.

Half-widths.  w <= 1e-3, and w >= 100 x the relative difference of the rule's quantity between device and oracle:

    parameter   step norms agree to 1e-6 relative (the trace tolerance of the parity tests)              -> w = 1e-4
    function    costs agree to 1e-9; at |cost change| / cost >= 1e-3 the ratio moves by <= 1e-6           -> w = 1e-4
    gradient    the parity tests bound the gradient relative to the LARGEST gradient of a run only, so the difference at the
                deciding iteration has to be measured: tests/test_lm_rules_gpu.py::test_gradient_margin prints it for every case
                that records a trace (with the step-norm and cost-ratio differences) and asserts w >= 100 x it.    -> w = 1e-3

Measured on an MI355X, relative difference |device - oracle| / oracle of the gradient max norm at the deciding iteration (trace
entry stop_at), as test_gradient_margin prints it, against w = 1e-3:

    main-plain 5.0e-9          main-xyzw-points 5.8e-9       main-inner 1.7e-7             main-intr-0x11 5.3e-10
    main-intr-0x3f 4.5e-10     main-mixed-models 5.0e-11     main-constant-blocks 1.1e-9   main-priors 9.5e-9
    invdepth-plain 1.9e-11     invdepth-intr-0x11 3.1e-9

(step norm: at most 5.4e-9, cost-change ratio: at most 1.7e-11, against w = 1e-4).  The batched loops record no trace: for them
test_batched_gradient_margin bisects the DEVICE's own critical gradient tolerance of problem 0 and prints it relative to the
oracle's t* (both bisected to 1e-6, which is the resolution of that figure; w / 100 = 1e-5).  Measured: below the resolution
(1.2e-8 printed) for the views, tracks, angular, homography and two-view BA loops; 2.6e-4 for the fundamental-matrix loop, whose
gradient rule is therefore not pinned (see its case).

Conditions on a case, each checked on the oracle by tests/test_lm_rule_cases.py: the rule's critical tolerance at stop_at and at
stop_at + 1 differ by a factor of ten or more; the designated problem's steps up to the stop were all accepted (never the noise
floor after convergence, where accept / reject is a rounding decision); for the function rule |cost change| / cost >= 1e-3 at
stop_at; for the gradient rule |cost change| / cost >= 1e-11 still at stop_at + 1, because the run at the lower bracket value
stops there only if that step is accepted -- further down the cost change is rounding noise (iteration 4 of most scenes: the
step ratio rho, and with it the new radius, then differ between device and oracle although both accept).  The two-view angular
and fundamental-matrix solves converge linearly for many iterations (their step roughly halves per iteration), so their cases sit
at the few (problem, iteration) pairs where the factor of ten exists.
"""
import functools
import math
from collections import namedtuple

import numpy as np

from pytheiasfm_amd import _capi as capi, synth
from tests import invdepth
from tests import oracle_lib as ol

RULES = ("function", "gradient", "parameter")
FIELD = {r: r + "_tolerance" for r in RULES}
W = {"function": 1e-4, "gradient": 1e-3, "parameter": 1e-4}

TERM_CONVERGENCE, TERM_NO_CONVERGENCE, TERM_FAILURE = 0, 1, 2

# What one problem's solve hands back: summary integers and costs, the trace (None where the loop records none) and the
# parameters as a tuple of arrays.
Result = namedtuple("Result", "success termination_type num_iterations num_successful_steps initial_cost final_cost trace params")


def result_of(s, trace, params):
    if isinstance(s, dict):
        s = namedtuple("S", s.keys())(**s)
    return Result(int(s.success), int(s.termination_type), int(s.num_iterations), int(s.num_successful_steps), float(s.initial_cost),
                  float(s.final_cost), trace, tuple(np.array(a, dtype=np.float64, copy=True) for a in params))


def tolerances(rule, value):
    """The other two tolerances at zero: only `rule` can yield CONVERGENCE before the cap."""
    t = {FIELD[r]: 0.0 for r in RULES}
    t[FIELD[rule]] = float(value)
    return t


def critical_tolerance(run, rule, stop_at, w=None, lo=1e-40, hi=1e30):
    """run(**tolerances) -> num_iterations of ONE problem.  Returns (t*, (t* (1 + w), t* (1 - w))) with t* the value of `rule`'s
    tolerance at which the run changes from stopping at iteration <= stop_at (tolerance above t*) to stopping later (below),
    bisected geometrically to 1e-6 relative.  [lo, hi] may be narrowed by the caller (the trace's own neighbouring values); a hint
    that does not enclose the flip is widened again.  Returns (None, None) when no tolerance stops the run by stop_at."""
    w = W[rule] if w is None else w
    early = lambda t: run(**tolerances(rule, t)) <= stop_at
    if not early(hi):
        hi = 1e30
        if not early(hi):
            return None, None
    if early(lo):
        lo = 1e-40
        if early(lo):
            return None, None
    while hi / lo > 1.0 + 1e-6:
        mid = math.sqrt(lo) * math.sqrt(hi)
        if early(mid):
            hi = mid
        else:
            lo = mid
    t = math.sqrt(lo) * math.sqrt(hi)
    return t, (t * (1.0 + w), t * (1.0 - w))


def options(default, fixed, **kw):
    o = default()
    for k, v in {**fixed, **kw}.items():
        setattr(o, k, v)
    return o


# ------------------------------------------------------------------ cases
class Case:
    """One loop on one scene.  problems(rule) builds the inputs once: a list of per-problem records, rolled so that the problem
    the bracket of `rule` is built from comes first ("problem 0"); oracle(rule, opt) runs the oracle of every problem on a copy
    and returns a list of Result (one entry for the single-problem loops).  The device side lives in the GPU test."""
    batch = False
    fixed = {}

    def __init__(self, name, stop_at, lead=(0, 0, 0), **kw):
        self.name = name
        self.stop_at = dict(zip(RULES, stop_at))
        self.lead = dict(zip(RULES, lead))
        self.w = dict(W)
        self.kw = kw

    def __repr__(self):
        return self.name

    def opt(self, default=ol.default_options, **kw):
        return options(default, self.fixed, **{**self.opt_kw(), **kw})

    def opt_kw(self):
        return {}

    @functools.lru_cache(maxsize=None)
    def scene(self):
        return self.build()

    def problems(self, rule):
        ps = self.scene()
        k = self.lead[rule]
        return ps[k:] + ps[:k]

    def oracle(self, rule, o, only=None):
        ps = self.problems(rule)
        return [self.oracle_one(p, o) for k, p in enumerate(ps) if only is None or k == only]

    @functools.lru_cache(maxsize=None)
    def critical(self, rule, stop_at=None):
        stop_at = self.stop_at[rule] if stop_at is None else stop_at
        run0 = lambda **kw: self.oracle(rule, self.opt(**kw), only=0)[0].num_iterations
        lo, hi = self.hint(rule, stop_at)
        return critical_tolerance(run0, rule, stop_at, self.w[rule], lo, hi)

    @functools.lru_cache(maxsize=None)
    def free_run(self, rule):
        """Problem 0 with all three tolerances at zero: runs to the cap (or the noise floor)."""
        return self.oracle(rule, self.opt(function_tolerance=0.0, gradient_tolerance=0.0, parameter_tolerance=0.0), only=0)[0]

    def fall(self, rule):
        """By how much the rule's quantity falls from stop_at to stop_at + 1: from the free run's trace where there is one (|x|
        hardly moves between two iterations, so the step norms stand for the parameter rule's quantity), else from two bisections."""
        k = self.stop_at[rule]
        tr = self.free_run(rule).trace
        if tr is None or tr.size <= k + 1:
            t, _ = self.critical(rule)
            t_next, _ = self.critical(rule, k + 1)
            return t / t_next if t and t_next else 0.0
        q = self.cost_change_ratio(rule) if rule == "function" else (tr.gradient_max_norm if rule == "gradient" else tr.step_norm)
        return q[k] / q[k + 1]

    def cost_change_ratio(self, rule):
        """|cost change| / cost per trace entry of the free run (entry 0: nan); the fixed cost of constant blocks is in both."""
        c = self.free_run(rule).trace.cost
        return np.concatenate([[np.nan], np.abs(np.diff(c)) / c[:-1]])

    def hint(self, rule, stop_at):
        """[lo, hi] from the free run's trace where there is one and its steps up to stop_at + 1 were all accepted."""
        tr = self.free_run(rule).trace
        if tr is None or tr.size <= stop_at + 1 or not tr.accepted[: stop_at + 2].all():
            return 1e-40, 1e30
        k = stop_at
        if rule == "gradient":
            q = tr.gradient_max_norm
            return q[k + 1] * 0.5, q[k] * 2.0
        if rule == "function":
            q = np.abs(np.diff(tr.cost)) / tr.cost[:-1]          # q[k - 1]: iteration k (the fixed cost shifts it slightly)
            return q[k] * 0.25, q[k - 1] * 4.0
        return 1e-40, 1e30

    @functools.lru_cache(maxsize=None)
    def expected(self, rule, side):
        """(tolerance, oracle results of every problem, problems to leave out) at bracket value `side` (0: t* (1 + w), 1: t* (1 - w)).
        Left out: the problems other than problem 0 whose own stop iteration changes anywhere between a guard value one more w
        above the bracket and one more w below it -- their own critical tolerance lies inside the bracket or at its edge."""
        t, pair = self.critical(rule)
        assert t is not None, (self.name, rule)
        w = self.w[rule]
        res = self.oracle(rule, self.opt(**tolerances(rule, pair[side])))
        skip = set()
        if self.batch:
            runs = [self.oracle(rule, self.opt(**tolerances(rule, v))) for v in (pair[0] * (1.0 + w), pair[0], pair[1], pair[1] * (1.0 - w))]
            for k in range(1, len(res)):
                if len({r[k].num_iterations for r in runs}) != 1:
                    skip.add(k)
        return pair[side], res, frozenset(skip)


class MainCase(Case):
    """theia_hip_ba_solve (ba_solver.hip, the device-resident control kernel) against oracle_ba_solve:
    synth_ba_v1(12, 300, seed=7), 3 intrinsics groups."""
    fixed = dict(max_num_iterations=12)
    scene_keys = ("mixed_models", "fix_gauge", "const", "priors", "start_scale", "focal_scale")

    def opt_kw(self):
        return {k: v for k, v in self.kw.items() if k not in self.scene_keys}

    def build(self):
        sc = self.kw.get("start_scale", 1.0)      # of the start perturbation (synth_ba_v1's defaults times sc)
        p = synth.synth_ba_v1(12, 300, seed=7, num_groups=3, mixed_models=self.kw.get("mixed_models", False),
                              fix_gauge=self.kw.get("fix_gauge", False), sigma_pos=0.05 * sc, sigma_rot_deg=0.5 * sc, sigma_pt=0.02 * sc)
        p.intrinsics[:, 0] *= self.kw.get("focal_scale", 1.0)
        if self.kw.get("const"):      # cam_const as in test_constant_blocks_fixed_cost_and_masks, every fourth point constant
            p.cam_const = np.array([3, 0, 1, 2, 0, 0, 3, 0, 0, 0, 4, 0], np.uint8)
            pc = np.zeros(300, np.uint8); pc[::4] = 1
            p.point_const = pc
        if self.kw.get("priors"):
            from tests.test_ba_gpu import _with_priors
            _with_priors(p, 0x9A12)
        return [p]

    def oracle_one(self, p, o):
        p = p.copy()
        s, tr = ol.solve(p, o)
        return result_of(s, tr, (p.cam_ext, p.points, p.intrinsics))


class InvDepthCase(Case):
    """The inverse-depth path (ba_invdepth.hip, id_handle_run) against oracle_ba_solve_inverse_depth: invdepth.make(8, 200)."""
    fixed = dict(max_num_iterations=12, use_inner_iterations=0)

    scene_keys = ("focal_scale", "const", "advance")

    def opt_kw(self):
        return {k: v for k, v in self.kw.items() if k not in self.scene_keys}

    def build(self):
        p = invdepth.make(8, 200, seed=5)
        p.intrinsics[:, 0] *= self.kw.get("focal_scale", 1.0)
        if self.kw.get("const"):      # masks as in test_invdepth_gpu.py: a constant camera, a constant position, every 11th depth
            p.cam_const = np.zeros(8, np.uint8); p.cam_const[0] = 3; p.cam_const[5] = 1
            p.point_const = np.zeros(200, np.uint8); p.point_const[::11] = 1
        if self.kw.get("advance"):    # start from where the oracle is after that many iterations: the first step is then small
            free = dict(function_tolerance=0.0, gradient_tolerance=0.0, parameter_tolerance=0.0)
            ol.solve_inverse_depth(p, self.opt(max_num_iterations=self.kw["advance"], **free))
        return [p]

    def oracle_one(self, p, o):
        p = p.copy()
        s, tr = ol.solve_inverse_depth(p, o)
        return result_of(s, tr, (p.cam_ext, p.point_inverse_depth, p.intrinsics))


class ViewsCase(Case):
    """theia_hip_ba_views_batch (ba_batch.hip): the scenes of _view_batch, 8 problems over the models (0, 5, 2, 1), each against
    oracle_ba_solve on its one-camera problem."""
    batch = True
    fixed = dict(max_num_iterations=15, use_homogeneous_point_parametrization=0, use_inner_iterations=0)

    def build(self):
        from tests.test_ba_gpu import _view_batch
        num = 8
        offs, obs, Xs, cams, intr, mods, truth = _view_batch(num, 0xBA7C, models=(0, 5, 2, 1))
        oo = ol.default_options()
        out = []
        for k in range(num):      # observations: the oracle's projection at the true pose + noise (as the parity test)
            model, kk, ext, X4, nz = obs[k]
            n = X4.shape[0]
            fp = capi.FlatProblem(ext[None].copy(), kk[None].copy(), np.array([model], np.int32), np.array([0], np.int32), X4.copy(),
                                  np.zeros((n, 2)), np.zeros(n, np.int32), np.arange(n, dtype=np.int32), point_const=np.ones(n, np.uint8))
            _, _, r, _, _ = ol.evaluate(fp, oo)
            fp.obs_uv = r + nz; fp.cam_ext = cams[k][None].copy()
            out.append(dict(uv=fp.obs_uv.copy(), points=X4, cam=cams[k].copy(), intr=intr[k], model=mods[k], flat=fp))
        return out

    def oracle_one(self, p, o):
        q = p["flat"].copy()
        s, tr = ol.solve(q, o)
        return result_of(s, tr, (q.cam_ext[0],))


class TracksCase(Case):
    """theia_hip_ba_tracks_batch (ba_batch.hip): synth_ba_v1(16, 120, mixed models, sigma_pt=0.05); the launch solves all 120
    tracks, eight of them are compared with oracle_ba_solve on "this point variable, everything else constant"."""
    batch = True
    fixed = dict(max_num_iterations=20, use_inner_iterations=0)
    tracks = (0, 7, 14, 21, 28, 35, 42, 49)

    def opt_kw(self):
        return dict(use_homogeneous_point_parametrization=self.kw["manifold"])

    @functools.lru_cache(maxsize=None)
    def flat(self):
        return synth.synth_ba_v1(16, 120, seed=0x7AC5, mixed_models=True, sigma_pt=0.05)

    def build(self):
        return list(self.tracks)

    def oracle_one(self, q, o):
        p = self.flat()
        sel = p.obs_pt == q
        fp = capi.FlatProblem(p.cam_ext.copy(), p.intrinsics.copy(), p.group_model, p.cam_group, p.points[q:q + 1].copy(), p.obs_uv[sel],
                              p.obs_cam[sel], np.zeros(sel.sum(), np.int32), cam_const=np.full(p.cam_ext.shape[0], 3, np.uint8))
        s, tr = ol.solve(fp, o)
        return result_of(s, tr, (fp.points[0],))


class AngularCase(Case):
    """theia_hip_ba_two_views_angular_batch (twoview_lm.hip), CGNR or exact steps, against oracle_two_views_angular: the first
    eight pairs of the scene of test_two_views_angular_batch_follows_oracle.  These solves converge linearly (the step roughly halves
    per iteration), so the designated problem and stop_at of each rule are the ones where the factor of ten exists; for the
    parameter rule that needs other seeds of the same generator (the "-b" cases, which pin that rule alone)."""
    batch = True
    fixed = dict(max_num_iterations=15, loss_function_type=0, robust_loss_width=1.0)

    def build(self):
        num = 8
        data, off, truth = synth.synth_ransac_v1(num, 500, kind="relative", noise_px=self.kw.get("noise_px", 0.5), seed=self.kw.get("seed", 0x5AC50C00))
        out = []
        for p in range(num):
            c = data[off[p]:off[p + 1]][truth["inlier"][p]]
            w = synth.matrix_to_angle_axis(truth["R"][p]); pos = truth["position"][p] / np.linalg.norm(truth["position"][p])
            x0 = np.concatenate([w + 0.004 * (p % 3 + 1), pos + 0.01 * ((p % 4) - 1.5)]); x0[3:] /= np.linalg.norm(x0[3:])
            out.append(dict(corr=c, x0=x0))
        return out

    def oracle_one(self, p, o):
        pose, s = ol.two_views_angular(p["corr"], p["x0"], o, self.kw["solver"])
        return result_of(s, None, (pose,))


class HomographyCase(Case):
    """theia_hip_optimize_homography_batch (twoview_lm.hip) against oracle_optimize_homography: the scenes of
    test_optimize_homography_batch_and_lo_follow_oracle, eight of them."""
    batch = True
    fixed = dict(max_num_iterations=15, loss_function_type=0)

    def build(self):
        from tests.test_oracle_ransac import _homography_scene
        out = []
        for k in range(8):
            H, c = _homography_scene(20 + k, n=100 + 30 * k)
            out.append(dict(corr=c, x0=H * (1.0 + 0.3 * k) + np.array([[0.01, -0.01, 2.0 + k], [0.01, 0.0, -2.0], [1e-6, 0, 0.0]])))
        return out

    def oracle_one(self, p, o):
        H, s = ol.optimize_homography(p["corr"], p["x0"], o)
        return result_of(s, None, (H,))


class FundamentalCase(Case):
    """theia_hip_optimize_fundamental_matrix_batch (twoview_lm.hip) against oracle_optimize_fundamental: the scenes of
    test_optimize_fundamental_matrix_batch_and_lo_follow_oracle, eight of them.  As the angular solves these converge linearly for
    many iterations: designated problem and stop_at per rule are where the factor of ten exists."""
    batch = True
    fixed = dict(max_num_iterations=12)

    def build(self):
        from tests.test_oracle_ransac import _fundamental_scene
        out = []
        for k in range(8):
            F, c = _fundamental_scene(0x5AC52500 + k, n=120 + 20 * k)
            out.append(dict(corr=c, x0=F * (1.0 + k) + (k + 1) * 1e-8 * np.array([[1.0, -2, 300], [2, 1, -200], [-300, 200, 5e4]])))
        return out

    def oracle_one(self, p, o):
        F, s = ol.optimize_fundamental(p["corr"], p["x0"], o)
        return result_of(s, None, (F,))


class TwoViewBaCase(Case):
    """theia_hip_ba_two_views_batch (twoview_ba.hip): N x BundleAdjustTwoViews against oracle_ba_solve on the same flat problem
    (camera 1 constant, focal lengths free unless held, XYZW points without a manifold, no inner iterations): the ragged pairs
    of test_two_view_ba_batch_matches_the_general_solver and two more."""
    batch = True
    fixed = dict(max_num_iterations=20, intrinsics_to_optimize=0x01, use_homogeneous_point_parametrization=0, use_inner_iterations=0,
                 max_trust_region_radius=1e16)
    # (12, not the 8 of that test: with both focal lengths free an 8-point pair has 32 residuals for 32 unknowns beyond the
    # scale of each XYZW point; its cost heads for zero and a relative bound on the cost along the way means nothing)
    ns = (90, 40, 130, 64, 65, 12, 100, 33)

    def build(self):
        ns = self.ns
        data, offsets, truth = synth.synth_ransac_v1(len(ns), 130, "fundamental", seed=0x5AC52800, inlier_lo=1.0, inlier_hi=1.0, noise_px=0.5)
        out = []
        for i, n in enumerate(ns):
            corr = data[offsets[i]:offsets[i] + n]
            ext2 = np.concatenate([truth["position"][i] + 0.01, synth.matrix_to_angle_axis(truth["R"][i]) + 0.004])
            depth = 6.0 + 0.3 * np.sin(np.arange(n) + i)
            x1 = (corr[:, :2] - np.array([500.0, 400.0])) / 1000.0
            p3 = np.column_stack([x1 * depth[:, None], depth, np.ones(n)])
            const = (int(i % 2 == 0), int(i % 3 == 0))
            intr = np.zeros((2, capi.THEIA_MAX_INTRINSICS)); intr[0, :5] = [1000.0, 1, 0, 500, 400]; intr[1, :5] = [1010.0, 1, 0, 500, 400]
            flat = capi.FlatProblem(np.array([np.zeros(6), ext2]), intr[:, :7].copy(), [0, 0], [0, 1], p3.copy(),
                                    np.concatenate([corr[:, :2], corr[:, 2:]]), np.concatenate([np.zeros(n, np.int32), np.ones(n, np.int32)]),
                                    np.concatenate([np.arange(n), np.arange(n)]).astype(np.int32), cam_const=[3, 0], group_const=list(const))
            out.append(dict(corr=corr, cam_ext=np.array([np.zeros(6), ext2]), intr=intr, const=const, points=p3, flat=flat))
        return out

    def oracle_one(self, p, o):
        q = p["flat"].copy()
        s, tr = ol.solve(q, o)
        return result_of(s, tr, (q.cam_ext[1], q.intrinsics[:, 0], q.points))


# stop_at (and, for the batches, the designated problem) per rule in the order (function, gradient, parameter); None: the case does
# not pin that rule.  Chosen on the oracle
# where each rule's critical tolerance falls by ten or more to the next iteration; the function rule where it is still >= 1e-3.
MAIN_CASES = [
    MainCase("main-plain", (2, 2, 3), use_inner_iterations=0),
    MainCase("main-xyzw-points", (2, 2, 3), use_inner_iterations=0, use_homogeneous_point_parametrization=0),
    MainCase("main-inner", (1, 2, 3), use_inner_iterations=1),
    # focal lengths 2 % off at the start: the first accepted step then moves x_norm by 1 % (100 w), so an x_norm that is not
    # refreshed after an accepted step stops elsewhere; on the other scenes x_norm moves by 1e-6 .. 3e-4 only
    MainCase("main-intr-0x11", (2, 2, 3), use_inner_iterations=0, intrinsics_to_optimize=0x11, focal_scale=1.02),
    # with every intrinsic free the scene needs its gauge fixed to converge quadratically at all
    MainCase("main-intr-0x3f", (2, 3, 4), use_inner_iterations=0, intrinsics_to_optimize=0x3f, fix_gauge=True),
    MainCase("main-mixed-models", (2, 2, 3), use_inner_iterations=0, mixed_models=True),
    MainCase("main-constant-blocks", (2, 2, 3), use_inner_iterations=0, const=True),
    MainCase("main-priors", (2, 3, 4), use_inner_iterations=0, priors=True, prior_mask=7),
    # a parameter-tolerance stop at the FIRST iteration is the only reader of the x_norm summed before the loop (k_xnorm_*; after an
    # accepted step it comes from the back-substitution's sums): free intrinsics, constant points, partly constant cameras, and a
    # start close enough (a tenth of the usual perturbation) for the second step to be ten times smaller than the first
    MainCase("main-first-step", (None, None, 1), use_inner_iterations=0, intrinsics_to_optimize=0x11, const=True, start_scale=0.1),
]
INVDEPTH_CASES = [
    InvDepthCase("invdepth-plain", (2, 2, 3)),
    InvDepthCase("invdepth-intr-0x11", (2, 3, 3), intrinsics_to_optimize=0x11, focal_scale=1.02),      # (as main-intr-0x11)
    # as main-first-step: id_handle_run reads the x_norm of k_id_xnorm only until the first accepted step (ID_XNORMSQ afterwards).
    # Free intrinsics, constant depths and cameras; the start is the oracle's state after one iteration, so that the second step
    # is ten times smaller than the first
    InvDepthCase("invdepth-first-step", (None, None, 1), intrinsics_to_optimize=0x11, const=True, advance=1),
]
BATCH_CASES = [
    ViewsCase("views-batch", (1, 2, 2)),
    TracksCase("tracks-batch-manifold", (1, 2, 2), manifold=1),
    TracksCase("tracks-batch-xyzw", (1, 2, 2), manifold=0),
    AngularCase("angular-cgnr", (4, 4, None), lead=(0, 1, 0), solver=1),
    AngularCase("angular-cgnr-b", (None, None, 7), lead=(0, 0, 5), solver=1, seed=0x5AC50C02, noise_px=0.1),
    AngularCase("angular-exact", (5, 4, None), lead=(1, 7, 0), solver=0),
    AngularCase("angular-exact-b", (None, None, 3), lead=(0, 0, 0), solver=0, seed=0x5AC50C05),
    HomographyCase("homography", (1, 2, 3)),
    # no gradient case: the only (problem, iteration) with a factor of ten is problem 1 at iteration 2, and there the device's
    # critical gradient tolerance, bisected by test_batched_gradient_margin, lay 2.6e-4 relative off the oracle's (F agreed to
    # 1e-16): the projected gradient |x - Plus(x, -g)| of a gradient of 1e11 is an ill-conditioned number.  w >= 100 x 2.6e-4
    # is more than the 1e-3 allowed and there is no earlier iteration, so the rule stays unpinned for this loop.
    FundamentalCase("fundamental", (10, None, 1), lead=(0, 0, 0)),
    TwoViewBaCase("two-view-ba", (3, 3, 3)),
    # a parameter stop at iteration 1 reads the x_norm each wavefront loop sets up before its first step (fundamental-parameter
    # above is one too).  The angular and two-view BA loops have no first step ten times their second: theirs stays unpinned.
    ViewsCase("views-batch-first-step", (None, None, 1)),
    TracksCase("tracks-batch-manifold-first-step", (None, None, 1), manifold=1),
    TracksCase("tracks-batch-xyzw-first-step", (None, None, 1), manifold=0),
    HomographyCase("homography-first-step", (None, None, 1)),
]
CASES = MAIN_CASES + INVDEPTH_CASES + BATCH_CASES
CASE_RULES = [(c, r) for c in CASES for r in RULES if c.stop_at[r] is not None]
TRACED_CASES = MAIN_CASES + INVDEPTH_CASES
# independent_lm.solve restates the pinhole main solve without inner iterations (no constant masks beyond whole cameras)
INDEPENDENT_CASES = [c for c in MAIN_CASES if c.name in ("main-plain", "main-xyzw-points", "main-intr-0x11")]
