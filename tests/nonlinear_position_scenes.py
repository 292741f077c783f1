"""The scenes of the NONLINEAR position stage's tests (tests/test_nonlinear_positions.py checks on the CPU that the
restatement alone reaches the branches each scene is meant to reach, with every decision margin above 1e-3;
tests/test_nonlinear_positions_gpu.py runs the device on them), and a cache of the restatement's solves, which the two
share within one process."""
import numpy as np

from pytheiasfm_amd.synth import angle_axis_to_matrix
from tests import nonlinear_position_ref as ref

_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _pairs(n, E, rng, star=False):
    """E distinct pairs over n views: a chain first (a star's spokes first), then random ones; the order is shuffled."""
    chosen = [(0, k) for k in range(1, n)] if star else [(k, k + 1) for k in range(n - 1)]
    if star:
        chosen += [(k, k + 1) for k in range(1, n - 1)]
    have = set(chosen)
    while len(chosen) < E:
        a, b = sorted(int(v) for v in rng.choice(n, 2, replace=False))
        if (a, b) not in have:
            have.add((a, b)); chosen.append((a, b))
    e = np.array(chosen[:max(E, len(chosen))], dtype=np.int32)
    e = e[rng.permutation(len(e))]
    flip = rng.random(len(e)) < 0.3                     # a pair may be named (larger, smaller)
    e[flip] = e[flip][:, ::-1]
    return e


def camera_scene(n, E, seed, noise_deg=1.0, outliers=0.0, scale_every=0, start="near", star=False):
    """n views at N(0, 5^2) positions with orientations over a wide range; position_2 = R_i (c_j - c_i) / |.| turned by
    noise_deg of noise, a share `outliers` of them replaced by random directions; every scale_every-th pair carries its
    true baseline as scale estimate.  start: "near" = the truth moved by N(0, 0.05^2), "random" = 100 U(-1, 1)."""
    rng = np.random.default_rng(seed)
    gt = rng.normal(0.0, 5.0, (n, 3))
    aa = rng.uniform(-1.5, 1.5, (n, 3))
    e = _pairs(n, E, rng, star)
    R = angle_axis_to_matrix(aa)
    d = gt[e[:, 1]] - gt[e[:, 0]]
    base = np.linalg.norm(d, axis=1)
    rel = np.einsum("eij,ej->ei", R[e[:, 0]], _unit(d))
    rel = _unit(rel + np.tan(np.radians(noise_deg)) * rng.normal(0.0, 1.0, rel.shape) / np.sqrt(3.0))
    bad = np.zeros(len(e), dtype=bool)
    bad[rng.permutation(len(e))[:int(round(outliers * len(e)))]] = True
    rel[bad] = _unit(rng.normal(0.0, 1.0, (int(bad.sum()), 3)))
    scales = None
    if scale_every:
        scales = -np.ones(len(e))
        scales[::scale_every] = base[::scale_every]
    init = gt + rng.normal(0.0, 0.05, gt.shape) if start == "near" else 100.0 * rng.uniform(-1.0, 1.0, gt.shape)
    return dict(aa=aa, gt=gt, init=init, edges=e, rel=rel, scales=scales, outliers=bad, kw={})


def point_scene(seed, n=5, T=8):
    """n views near the plane z = 0 looking down +z, T points at depth 8 .. 12, every point seen by three views or more.
    The features are those of the true orientations, which go in as ray_orientations; the solve's orientations are the
    truth turned by about a degree, as estimated ones are."""
    rng = np.random.default_rng(seed)
    s = camera_scene(n, 7, seed, noise_deg=0.5)
    s["gt"] = np.column_stack([rng.uniform(-2.0, 2.0, (n, 2)), rng.uniform(-0.3, 0.3, n)])
    ray_aa = rng.uniform(-0.25, 0.25, (n, 3))
    s["aa"] = ray_aa + rng.normal(0.0, 0.015, (n, 3))
    R = angle_axis_to_matrix(s["aa"])
    d = s["gt"][s["edges"][:, 1]] - s["gt"][s["edges"][:, 0]]
    s["rel"] = _unit(np.einsum("eij,ej->ei", R[s["edges"][:, 0]], _unit(d)) + rng.normal(0.0, 0.005, (len(d), 3)))
    X = np.column_stack([rng.uniform(-3.0, 3.0, (T, 2)), rng.uniform(8.0, 12.0, T)])
    Rr = angle_axis_to_matrix(ray_aa)
    offsets, ov, of = [0], [], []
    for t in range(T):
        for v in sorted(int(k) for k in rng.choice(n, int(rng.integers(3, n + 1)), replace=False)):
            p = Rr[v] @ (X[t] - s["gt"][v])
            ov.append(v); of.append(p[:2] / p[2] + rng.normal(0.0, 1e-3, 2))
        offsets.append(len(ov))
    s["init"] = s["gt"] + rng.normal(0.0, 0.05, s["gt"].shape)
    s["kw"] = dict(points=X + rng.normal(0.0, 0.1, X.shape), track_offsets=np.array(offsets, dtype=np.int32),
                   obs_view=np.array(ov, dtype=np.int32), obs_feature=np.array(of), ray_orientations=ray_aa,
                   point_to_camera_weight=0.5 * len(s["edges"]) / len(ov))
    s["points_gt"] = X
    return s


def _tiny3():
    s = camera_scene(3, 3, 5)
    s["init"][1] = s["init"][0]                          # |x_1 - x_0| = 0 < 1e-12 at iteration 0
    return s


def _far8():
    s = camera_scene(8, 20, 8, scale_every=1)            # every pair has a scale: the gauge is a translation alone
    s["init"] = 0.5 * s["gt"] + 0.05
    return s


def _held30():
    s = camera_scene(30, 299, 3)
    s["edges"] = np.concatenate([s["edges"], np.array([[3, 7]], dtype=np.int32)])       # both ends held
    s["rel"] = np.concatenate([s["rel"], [[0.0, 0.6, 0.8]]])
    fixed = np.zeros(30, dtype=bool); fixed[[3, 7, 20]] = True
    s["kw"] = dict(fixed=fixed)
    return s


def _no_edge():
    s = camera_scene(4, 5, 1)
    s["aa"] = np.concatenate([s["aa"], [[0.1, 0.2, 0.3]]]); s["init"] = np.concatenate([s["init"], [[7.0, 7.0, 7.0]]])
    return s


def _all_held():
    s = camera_scene(4, 5, 1)
    s["kw"] = dict(fixed=np.ones(4, dtype=bool))
    return s


# name -> (builder, what the restatement must meet on it: `seen` flags, a long run, at least one rejected step)
CASES = {
    "n4": (lambda: camera_scene(4, 5, 1), dict(seen=("normalised",), order=12)),
    "n6_scales": (lambda: camera_scene(6, 10, 2, scale_every=2), dict(seen=("normalised", "scaled"), order=18)),
    "tiny3": (_tiny3, dict(seen=("tiny", "outlier"), order=9, long=True)),
    "out10": (lambda: camera_scene(10, 25, 4, noise_deg=2.0, outliers=0.3, start="random"),
              dict(seen=("inlier", "outlier"), order=30, long=True, rejected=True)),
    "far8_scales": (_far8, dict(seen=("scaled", "inlier", "outlier"), order=24, long=True)),
    "pts5": (lambda: point_scene(6), dict(seen=("normalised",), order=39)),
    "n30": (lambda: camera_scene(30, 300, 3), dict(seen=("normalised",), order=90)),
    "star70": (lambda: camera_scene(71, 139, 7, star=True), dict(seen=("normalised",), order=213)),
    "held30": (_held30, dict(seen=("normalised",), order=81)),
    "no_edge": (_no_edge, dict(seen=("normalised",), order=12)),
    "all_held": (_all_held, dict(seen=(), order=0)),
}


def scene(name):
    return cached(("scene", name), CASES[name][0])


def reference(name, **kw):
    key = ("ref", name, tuple(sorted((k, v if np.isscalar(v) else tuple(np.asarray(v).tolist())) for k, v in kw.items())))

    def make():
        s = scene(name)
        return ref.solve(s["aa"], s["init"], s["edges"], s["rel"], s["scales"], **{**s["kw"], **kw})
    return cached(key, make)


# ---- the stopping rules reached in turn, on "n4" / "n30" / "far8_scales" (as tests/test_nonlinear_rotations_gpu.py reaches them)
def _between(a, b):
    assert a > 0.0 and b > 0.0 and a != b
    return float(np.sqrt(a * b))


def stopping_case(kind):
    """(scene name, solve keywords, the termination and the iteration count the restatement must give)."""
    if kind.startswith("cap"):
        cap = int(kind[3:])
        return "n4", dict(max_num_iterations=cap), ref.TERM_CAP, cap
    if kind == "function":
        return "n30", {}, ref.TERM_FUNCTION, reference("n30")["iterations"]
    if kind == "gradient":                               # below the start's gradient, above the first step's
        base = reference("n30")
        assert base["gmaxs"][1] < base["gmaxs"][0]
        return "n30", dict(gradient_tolerance=_between(base["gmaxs"][0], base["gmaxs"][1])), ref.TERM_GRADIENT, 1
    if kind == "parameter1":                             # the first step's ratio to the initial |x|, and ten times it
        base = reference("n30")
        ratio = base["step_norms"][0] / base["x_norms"][0]
        return "n30", dict(parameter_tolerance=_between(ratio, 10.0 * ratio)), ref.TERM_PARAMETER, 1
    if kind == "parameter2":                             # the first step passes, the second stops on the refreshed |x|
        base = reference("far8_scales", function_tolerance=0.0)
        r1, r2 = base["step_norms"][0] / base["x_norms"][0], base["step_norms"][1] / base["x_norms"][1]
        assert r2 < r1
        return "far8_scales", dict(function_tolerance=0.0, parameter_tolerance=_between(r1, r2)), ref.TERM_PARAMETER, 2
    raise KeyError(kind)


STOPPING_KINDS = ("cap0", "cap1", "cap3", "function", "gradient", "parameter1", "parameter2")


# ---- the mirror: a reconstruction, view pairs and orientations for NonlinearPositionEstimator
def mirror_case(seed=6):
    """The views and tracks of point_scene(seed) as an sfm.Reconstruction with non-trivial view ids left to the caller:
    (reconstruction, normalised features per observation, {(i, j): TwoViewInfo}, {view: angle-axis}, scene).  Track 7
    is un-estimated; every second pair carries a scale estimate."""
    from pytheiasfm_amd import sfm
    from pytheiasfm_amd.twoview import TwoViewInfo
    s = point_scene(seed)
    kw = s["kw"]
    n, T = len(s["gt"]), len(s["points_gt"])
    r = sfm.Reconstruction()
    r.cam_ext = np.column_stack([s["init"], kw["ray_orientations"]])
    r.view_estimated = np.ones(n, dtype=bool)
    r.points = np.column_stack([2.0 * kw["points"], 2.0 * np.ones(T)])       # homogeneous, w = 2
    r.track_estimated = np.ones(T, dtype=bool); r.track_estimated[7] = False
    r.obs_view = kw["obs_view"].copy()
    r.obs_track = np.repeat(np.arange(T), np.diff(kw["track_offsets"])).astype(np.int32)
    r.obs_uv = kw["obs_feature"].copy()
    pairs = {}
    for k, ((a, b), t) in enumerate(zip(s["edges"], s["rel"])):
        info = TwoViewInfo()
        info.position_2 = np.array(t)
        if k % 2 == 0:
            info.scale_estimate = float(np.linalg.norm(s["gt"][b] - s["gt"][a]))
        pairs[(int(a), int(b))] = info
    return r, kw["obs_feature"].copy(), pairs, {v: s["aa"][v].copy() for v in range(n)}, s


def restatement_as_device(orientations, positions, edges, relative_translations, scale_estimates=None, fixed=None,
                          points=None, track_offsets=None, obs_view=None, obs_feature=None, ray_orientations=None,
                          point_to_camera_weight=0.5, options=None, want_trace=False):
    """global_pose.nonlinear_positions' signature on the restatement, for the mirror's tests without a device; the
    summary carries the counts, `restatement_as_device.last` the restatement's dict."""
    from pytheiasfm_amd import _capi as capi
    o = ref.solve(orientations, positions, edges, relative_translations, scale_estimates, fixed, points, track_offsets,
                  obs_view, obs_feature, ray_orientations, point_to_camera_weight, options.robust_loss_width,
                  options.max_num_iterations, options.function_tolerance, options.gradient_tolerance,
                  options.parameter_tolerance, options.max_trust_region_radius)
    restatement_as_device.last = o
    restatement_as_device.args = dict(orientations=orientations, positions=positions, edges=edges, rel=relative_translations,
                                      scales=scale_estimates, fixed=fixed, points=points, track_offsets=track_offsets,
                                      obs_view=obs_view, obs_feature=obs_feature, ray_orientations=ray_orientations,
                                      weight=point_to_camera_weight)
    s = capi.NonlinearPositionSummary()
    s.iterations, s.termination = o["iterations"], o["term"]
    s.num_successful_steps, s.num_unsuccessful_steps, s.num_invalid_steps = o["successful"], o["unsuccessful"], o["invalid"]
    return 0, o["x"].copy(), o["points"].copy(), s
