"""Small deterministic BA scenes whose START state sits on the branch edges of the device code (test side only).

edge_scene(model, seed) is a ring of 12 cameras in three intrinsics groups and about 210 tracks of 2 .. 10 observations:
the smallest shape that still gives the fused plan several runs, every track length of a wave tile and all groups in use.
Observations are the ORACLE's projection of the true state (oracle evaluate with obs_uv = 0) plus 0.5 px noise; the start
state is the truth perturbed, with the following planted in it:

  * camera 0 has an exactly zero angle-axis and camera 1 one of norm 1e-9 (the first-order branch of the rotation,
    theta^2 <= DBL_EPSILON); they stand next to each other, see the common cloud and share ten tracks of their own;
  * one point at the world origin (Householder: sigma <= DBL_EPSILON), one with w = 0.25 (a scaled homogeneous vector);
  * for the models where a flipped q stays valid (0, 1, 3, 4) one point with w = -1 (Householder: w <= 0);
  * three points on the optical axis of each of the cameras 2, 3 and 4 (one camera per group), seen by the neighbours too:
    the FOV model's ru^2 < 1e-3 series and the fisheye model's on-axis case r^2 < 1e-8;
  * per model, intrinsics groups on both sides of each branch: FOV omega 0.9 / 5e-4 / 0.7, division k -1e-7 / 0 / 4e-6
    (with four far off-axis points so that 1 - 4 k ru^2 < 0 occurs), double sphere alpha 0.55 / 0.3 / 0.6, extended
    unified alpha 0.6 / 0.4 / 0.55;
  * for the fisheye model four points BEHIND two cameras (z < 0), seen from the other side of the ring as well.

branch_counts() restates every branch condition in numpy on the start state, so that a test can assert that the scene
really takes them.  invalid_candidate_scene() is the scene of the rejected-candidate test (see there)."""
import functools

import numpy as np

from pytheiasfm_amd import _capi as capi
from tests import oracle_lib as ol

NV = 12
EPS = np.finfo(np.float64).eps

# three intrinsics groups per model (group = camera index mod 3)
INTRINSICS = {
    0: [[1000.0, 1.0, 0.0, 960.0, 540.0, -0.05, 0.01], [980.0, 1.01, 0.1, 950.0, 545.0, -0.04, 0.008], [1020.0, 0.99, -0.1, 965.0, 535.0, -0.06, 0.012]],
    1: [[1000.0, 1.02, 0.2, 960.0, 540.0, -0.1, 0.02, 0.001, 0.001, -0.002], [990.0, 1.0, 0.1, 955.0, 542.0, -0.08, 0.015, 0.002, -0.001, 0.001],
        [1010.0, 0.98, 0.0, 962.0, 538.0, -0.12, 0.025, 0.0, 0.002, 0.002]],
    2: [[600.0, 1.0, 0.1, 960.0, 540.0, 0.01, -0.002, 0.001, 0.0005], [610.0, 1.01, 0.0, 955.0, 545.0, 0.02, -0.003, 0.0005, 0.0002],
        [590.0, 0.99, 0.05, 965.0, 535.0, -0.01, 0.001, 0.0, 0.0]],
    3: [[800.0, 1.01, 960.0, 540.0, 0.9], [810.0, 1.0, 955.0, 545.0, 5e-4], [790.0, 0.99, 965.0, 535.0, 0.7]],
    4: [[1000.0, 0.99, 960.0, 540.0, -1e-7], [990.0, 1.0, 955.0, 545.0, 0.0], [1010.0, 1.01, 965.0, 535.0, 4e-6]],
    5: [[600.0, 1.0, 0.0, 960.0, 540.0, -0.2, 0.55], [610.0, 1.01, 0.1, 955.0, 545.0, -0.2, 0.3], [590.0, 0.99, 0.0, 965.0, 535.0, 0.1, 0.6]],
    6: [[600.0, 1.0, 0.0, 960.0, 540.0, 0.6, 1.1], [610.0, 1.01, 0.1, 955.0, 545.0, 0.4, 1.1], [590.0, 0.99, 0.0, 965.0, 535.0, 0.55, 0.9]],
    7: [[80.0, 1.0, 0.1, 960.0, 540.0, 0.001, -0.0001], [82.0, 1.01, 0.0, 955.0, 545.0, 0.002, -0.0002], [78.0, 0.99, 0.05, 965.0, 535.0, 0.0005, 0.0]],
}
NEGATIVE_W_MODELS = (0, 1, 3, 4)


def angle_axis_to_matrix(w):
    """ceres AngleAxisRotatePoint as a matrix: Rodrigues if theta^2 > DBL_EPSILON, else I + [w]x."""
    w = np.asarray(w, dtype=np.float64)
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    th2 = float(w @ w)
    if th2 <= EPS:
        return np.eye(3) + K
    th = np.sqrt(th2)
    return np.eye(3) + np.sin(th) / th * K + (1.0 - np.cos(th)) / th2 * (K @ K)


def matrix_to_angle_axis(R):
    c = np.clip((np.trace(R) - 1.0) / 2.0, -1.0, 1.0)
    th = np.arccos(c)
    v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    if th < 1e-12:
        return 0.5 * v
    return th / (2.0 * np.sin(th)) * v     # (no camera of the ring comes near a half turn)


def _ring():
    """The start-state cameras: 0 and 1 unrotated at z = -7 looking along +z, 2 .. 11 on the ring around the y axis, looking
    at the origin."""
    cams = np.zeros((NV, 6))
    cams[0] = [0.35, 0.1, -7.0, 0.0, 0.0, 0.0]
    cams[1] = [-0.45, -0.15, -7.3, 6e-10, -8e-10, 0.0]
    for c in range(2, NV):
        a = np.deg2rad(30.0 * (c - 1))
        pos = np.array([7.0 * np.sin(a), 0.4 * np.cos(3.0 * a), -7.0 * np.cos(a)])
        z = -pos / np.linalg.norm(pos)
        x = np.cross([0.0, 1.0, 0.0], z); x /= np.linalg.norm(x)
        R = np.stack([x, np.cross(z, x), z])
        cams[c] = np.concatenate([pos, matrix_to_angle_axis(R)])
    return cams


def camera_frame(cam_ext, points, obs_cam, obs_pt):
    """q = R(w) (X - w C) of every observation, in numpy."""
    R = np.stack([angle_axis_to_matrix(c[3:]) for c in cam_ext])
    X = points[obs_pt]
    p = X[:, :3] - X[:, 3:4] * cam_ext[obs_cam, :3]
    return np.einsum("nij,nj->ni", R[obs_cam], p)


def model_valid(model, k, q):
    """The validity boolean of the camera models that have one (double sphere, extended unified), restated in numpy."""
    r2 = q[:, 0] ** 2 + q[:, 1] ** 2
    if model == 5:
        xi, al = k[:, 5], k[:, 6]
        d1 = np.sqrt(r2 + q[:, 2] ** 2)
        w1 = np.where(al > 0.5, (1.0 - al) / al, al / (1.0 - al))
        w2 = (w1 + xi) / np.sqrt(2.0 * w1 * xi + xi * xi + 1.0)
        return q[:, 2] > -w2 * d1
    if model == 6:
        al, be = k[:, 5], k[:, 6]
        n = al * np.sqrt(be * r2 + q[:, 2] ** 2) + (1.0 - al) * q[:, 2]
        with np.errstate(divide="ignore", invalid="ignore"):
            lim = (al - 1.0) / (al + al - 1.0)
            bad = (n < 1e-3) | ((al > 0.5) & (q[:, 2] / n < lim))
        return ~bad
    return np.ones(len(q), dtype=bool)


def project_with_oracle(p, cam_ext, points):
    """The oracle's projection of (cam_ext, points) on p's observation list: its residual at obs_uv = 0."""
    fp = capi.FlatProblem(cam_ext, p.intrinsics, p.group_model, p.cam_group, points, np.zeros_like(p.obs_uv), p.obs_cam, p.obs_pt)
    ok, _, r, _, _ = ol.evaluate(fp, ol.default_options())
    return ok, r


@functools.lru_cache(maxsize=None)
def _edge_scene(models, seed, perturb, negative_w):
    """models: the camera model of each of the three groups (edge_scene: the same three times)."""
    rng = np.random.default_rng([0xED6E, int(models[0]), int(seed)] + ([] if len(set(models)) == 1 else [int(m) for m in models[1:]]))
    cams = _ring()
    R = [angle_axis_to_matrix(c[3:]) for c in cams]
    pts, windows = [], []

    def add(X, first, length, w=1.0):
        pts.append(np.array([X[0] * w, X[1] * w, X[2] * w, w]))
        windows.append([(first + k) % NV for k in range(length)])

    add([0.0, 0.0, 0.0], 10, 5)                       # the world origin: cameras 10, 11, 0, 1, 2
    add([0.3, -0.2, 0.4], 0, 5, w=0.25)
    if negative_w:
        add([-0.25, 0.3, 0.2], 11, 5, w=-1.0)
    first_axis = len(pts)
    for c in (2, 3, 4):                               # on the optical axis of camera c: C + d R^T e_z
        for d in (6.2, 7.0, 7.9):
            add(cams[c, :3] + d * R[c][2], c - 1, 4)
    axis = list(range(first_axis, len(pts)))
    for k in range(10):                               # the tracks cameras 0 and 1 have to themselves
        add([1.6 * rng.random() - 0.8, 1.6 * rng.random() - 0.8, 1.0 + 1.5 * rng.random()], 0, 2)
    if 4 in models:                                   # far off the axis: 1 - 4 k ru^2 < 0 in the k = 4e-6 group
        for k, y in enumerate((2.6, -2.6, 2.9, -2.8)):
            add([0.2 * k - 0.3, y, 0.1 * k], 3 * k + 1, 4)
    nspecial = len(pts)
    for t in range(190):
        add(1.6 * rng.random(3) - 0.8, int(rng.integers(NV)), 2 + t % 9)
    if 2 in models:                                   # behind cameras 5 and 8 (z < 0), in front of the far side of the ring
        for k, c in enumerate((5, 8, 5, 8)):
            X = 1.35 * cams[c, :3] + np.array([0.3 * k - 0.4, 0.5 - 0.3 * k, 0.2])
            pts.append(np.append(X, 1.0)); windows.append([c, (c + 5) % NV, (c + 6) % NV, (c + 7) % NV])
    pts0 = np.array(pts)
    obs_cam = np.concatenate([np.asarray(w, np.int32) for w in windows])
    obs_pt = np.repeat(np.arange(len(pts), dtype=np.int32), [len(w) for w in windows])
    intr = np.zeros((3, capi.THEIA_MAX_INTRINSICS))
    for g, m in enumerate(models):
        k = INTRINSICS[m][g]
        intr[g, : len(k)] = k
    p = capi.FlatProblem(cams, intr, np.asarray(models, np.int32), np.arange(NV, dtype=np.int32) % 3, pts0,
                         np.zeros((len(obs_cam), 2)), obs_cam, obs_pt)
    # the truth: the start state moved by the perturbation (the planted values belong to the START state)
    cam_gt = cams.copy()
    cam_gt[:, :3] += 0.05 * perturb * rng.standard_normal((NV, 3))
    cam_gt[:, 3:] += np.deg2rad(0.5) * perturb * rng.standard_normal((NV, 3))
    pts_gt = pts0.copy()
    pts_gt[:, :3] += 0.02 * perturb * rng.standard_normal((len(pts), 3)) * pts0[:, 3:4]
    if negative_w and not set(models) <= set(NEGATIVE_W_MODELS):   # (the invalid-start scene: observed where the same 3-D point, w = +1, projects)
        pts_gt[pts_gt[:, 3] < 0.0] *= -1.0
    ok, uv = project_with_oracle(p, cam_gt, pts_gt)
    assert ok == 1, "the true state must be valid in every observation"
    p.obs_uv = np.ascontiguousarray(uv + 0.5 * rng.standard_normal(uv.shape))
    return p, {"planted": nspecial, "origin": 0, "axis": axis}


def off_the_edges(p):
    """p with the point at the origin moved to (1, -2, 1.5) e-3 and the on-axis points moved 1e-3 sideways.  With the AMBIENT
    parametrisation (PD 4) those two plants leave a point block singular up to the LM floor -- the homogeneous scale of
    (0, 0, 0, w) is the w axis itself, whose Jacobian column is round-off -- and the ORACLE's own step then moves by up to
    O(1) relative when its input moves by 1e-15.  The Householder branch they stand for does not exist with PD 4; the
    camera-model branches of the on-axis points are still compared at the start state on the unmoved scene."""
    info = planted(p)
    q = p.copy()
    q.points[info["origin"]] = [1e-3, -2e-3, 1.5e-3, 1.0]
    q.points[info["axis"], :2] += 1e-3
    return q


def planted(p):
    """Indices of the planted points of an edge scene, read back from the scene itself."""
    sigma = (p.points[:, :3] ** 2).sum(1)
    origin = int(np.nonzero(sigma == 0.0)[0][0])
    q = camera_frame(p.cam_ext, p.points, p.obs_cam, p.obs_pt)
    on = (q[:, 0] ** 2 + q[:, 1] ** 2 < 1e-16) & np.isin(p.obs_cam, (2, 3, 4))
    return {"origin": origin, "axis": sorted(set(p.obs_pt[on].tolist()) - {origin})}


def edge_scene(model, seed=1, perturb=1.0, negative_w=None):
    """A fresh copy of the scene (FlatProblem).  perturb scales the distance of the start from the truth (the robust-loss
    cases start closer: ROBUST_PERTURB); negative_w plants the w = -1 point (default: the models where it stays valid)."""
    if negative_w is None:
        negative_w = model in NEGATIVE_W_MODELS
    return _edge_scene((int(model),) * 3, int(seed), float(perturb), bool(negative_w))[0].copy()


def mixed_scene(models=(0, 5, 3), constant_groups=(0, 0, 1), seed=1, perturb=1.0):
    """One camera model per group.  The default -- pinhole, double sphere and a CONSTANT FOV group -- is the only way to the
    FOCAL_LENGTH | RADIAL_DISTORTION instances of the all-models kernels: the free groups share the mask {0, 5, 6}, and the
    FOV group, which no mask could give those parameters, only brings its model into the kernel."""
    p = _edge_scene(tuple(int(m) for m in models), int(seed), float(perturb), False)[0].copy()
    p.group_const = np.asarray(constant_groups, np.uint8)
    return p


def branch_counts(p):
    """How many observations of p's START state take each branch of the device code, the conditions restated in numpy."""
    model = int(p.group_model[0])
    q = camera_frame(p.cam_ext, p.points, p.obs_cam, p.obs_pt)
    k = p.intrinsics[p.cam_group[p.obs_cam]]
    X = p.points[p.obs_pt]
    sigma = (X[:, :3] ** 2).sum(1)
    th2 = (p.cam_ext[p.obs_cam, 3:] ** 2).sum(1)
    out = {
        "rotation_small": int((th2 <= EPS).sum()), "rotation_exact_zero": int((th2 == 0.0).sum()),
        "rotation_rodrigues": int((th2 > EPS).sum()),
        "householder_sigma_small": int((sigma <= EPS).sum()),
        "householder_w_nonpositive": int(((sigma > EPS) & (X[:, 3] <= 0.0)).sum()),
        "householder_w_positive": int(((sigma > EPS) & (X[:, 3] > 0.0)).sum()),
        "w_quarter": int((X[:, 3] == 0.25).sum()),
    }
    with np.errstate(divide="ignore", invalid="ignore"):
        x, y = q[:, 0] / q[:, 2], q[:, 1] / q[:, 2]
    if model == 3:
        om, ru2 = k[:, 4], x * x + y * y
        out.update(fov_small_omega=int((om < 1e-3).sum()), fov_small_radius=int(((om >= 1e-3) & (ru2 < 1e-3)).sum()),
                   fov_general=int(((om >= 1e-3) & (ru2 >= 1e-3)).sum()))
    if model == 2:
        r2 = q[:, 0] ** 2 + q[:, 1] ** 2
        out.update(fisheye_on_axis=int((r2 < 1e-8).sum()), fisheye_behind=int(((r2 >= 1e-8) & (q[:, 2] < 0.0)).sum()),
                   fisheye_general=int(((r2 >= 1e-8) & (q[:, 2] >= 0.0)).sum()))
    if model == 5:
        out.update(ds_alpha_le_half=int((k[:, 6] <= 0.5).sum()), ds_alpha_gt_half=int((k[:, 6] > 0.5).sum()))
    if model == 6:
        out.update(eucm_alpha_le_half=int((k[:, 5] <= 0.5).sum()), eucm_alpha_gt_half=int((k[:, 5] > 0.5).sum()))
    if model == 4:
        ux, uy = k[:, 0] * x, k[:, 0] * k[:, 1] * y
        ru2 = ux * ux + uy * uy
        denom, inner = 2.0 * k[:, 4] * ru2, 1.0 - 4.0 * k[:, 4] * ru2
        out.update(division_denominator_zero=int((np.abs(denom) < EPS).sum()),
                   division_inner_negative=int(((np.abs(denom) >= EPS) & (inner < 0.0)).sum()),
                   division_general=int(((np.abs(denom) >= EPS) & (inner >= 0.0)).sum()),
                   division_min_general_inner=float(inner[(np.abs(denom) >= EPS) & (inner >= 0.0)].min()))
    out["invalid"] = int((~model_valid(model, k, q)).sum())
    return out


# ---------------------------------------------------------------- options of the cases
LOSSES = (0, 1, 2, 3, 4, 5, 6)       # trivial, Huber, SoftLOne, Cauchy, Arctan, Tukey, Truncated
LOSS_NAMES = ("trivial", "huber", "softlone", "cauchy", "arctan", "tukey", "truncated")
# The robust cases start at a fifth of the default distance from the truth and use a width of 4 px (8 px for the two
# losses whose weight falls to ZERO: Tukey beyond |r| = a, Truncated beyond |r|^2 = a): with the default start and width 1.5
# whole columns of the reduced system were left with nothing but the LM diagonal.  test_ba_edge_scenes.py asserts, with
# the oracle alone, that at most a quarter of the observations have a zero weight and that every camera and point keeps two.
ROBUST_PERTURB = 0.2
LOSS_WIDTH = {0: 1.0, 1: 4.0, 2: 4.0, 3: 4.0, 4: 4.0, 5: 8.0, 6: 8.0}


def case_scene(model, loss, seed=1):
    return edge_scene(model, seed, perturb=1.0 if loss == 0 else ROBUST_PERTURB)


def set_case(options, loss, pd, **kw):
    """The options of one case on an options struct of either side (device or oracle)."""
    options.use_homogeneous_point_parametrization = 1 if pd == 3 else 0
    options.loss_function_type = loss
    options.robust_loss_width = LOSS_WIDTH[loss]
    options.use_inner_iterations = 0
    for name, v in kw.items():
        setattr(options, name, v)
    return options


def zero_weight(loss, width, r):
    """rho' == 0 of the two losses that reach it, on the unweighted residuals r [n][2] (ceres TukeyLoss: s > a^2; the
    reference's TruncatedLoss: s >= a^2)."""
    s = (r ** 2).sum(1)
    if loss == 5:
        return s > width * width
    if loss == 6:
        return s >= width * width
    return np.zeros(len(s), dtype=bool)


def with_long_tracks(p, nlong=2, nobs=65):
    """p plus nlong tracks of nobs > 64 observations (the per-observation path): every camera sees them, the ring repeated
    until the track is long enough, as tests/test_ba_gpu._with_long_tracks does with more cameras."""
    rng = np.random.default_rng(0x10C6)
    X = np.column_stack([0.8 * rng.random((nlong, 3)) - 0.4, np.ones(nlong)])
    oc = np.tile(np.arange(nobs, dtype=np.int32) % NV, nlong)
    op = (p.points.shape[0] + np.repeat(np.arange(nlong), nobs)).astype(np.int32)
    q = capi.FlatProblem(p.cam_ext, p.intrinsics, p.group_model, p.cam_group, np.vstack([p.points, X]),
                         np.zeros((len(p.obs_cam) + len(oc), 2)), np.concatenate([p.obs_cam, oc]), np.concatenate([p.obs_pt, op]))
    ok, uv = project_with_oracle(q, q.cam_ext, q.points)
    assert ok == 1
    q.obs_uv[: len(p.obs_uv)] = p.obs_uv
    q.obs_uv[len(p.obs_uv):] = uv[len(p.obs_uv):] + 0.5 * rng.standard_normal((len(oc), 2))
    q.points[-nlong:, :3] += 0.02 * rng.standard_normal((nlong, 3))
    return q


def with_position_priors(p):
    """p with a position prior (THEIA_PRIOR_POSITION, sqrt information 20 I) on every camera, 0.02 off its start."""
    rng = np.random.default_rng(0x9A10)
    nc = p.cam_ext.shape[0]
    q = p.copy()
    q.set_priors(np.ones(nc, np.uint8), position=(p.cam_ext[:, :3] + 0.02 * rng.standard_normal((nc, 3)), np.tile(20.0 * np.eye(3), (nc, 1, 1))))
    return q


def camera_slices(p):
    """The scene as one localisation problem per camera (its observations against the start points, held constant):
    offsets, obs_uv, points [total][4], cam_ext [nc][6], intrinsics [nc][10], model [nc] for the views batch, and the same as
    one FlatProblem per camera for the oracle."""
    offs, uvs, Xs, flats = [0], [], [], []
    nc = p.cam_ext.shape[0]
    for c in range(nc):
        sel = p.obs_cam == c
        n = int(sel.sum())
        uvs.append(p.obs_uv[sel]); Xs.append(p.points[p.obs_pt[sel]]); offs.append(offs[-1] + n)
        g = p.cam_group[c]
        flats.append(capi.FlatProblem(p.cam_ext[c:c + 1].copy(), p.intrinsics[g:g + 1].copy(), p.group_model[g:g + 1], np.zeros(1, np.int32),
                                      Xs[-1].copy(), uvs[-1].copy(), np.zeros(n, np.int32), np.arange(n, dtype=np.int32),
                                      point_const=np.ones(n, np.uint8)))
    return (np.array(offs), np.vstack(uvs), np.vstack(Xs), p.cam_ext.copy(), p.intrinsics[p.cam_group].copy(),
            p.group_model[p.cam_group].astype(np.int32), flats)


def track_slice(p, t):
    """Track t of the scene as the oracle's problem "this point variable, every camera constant"."""
    sel = p.obs_pt == t
    return capi.FlatProblem(p.cam_ext.copy(), p.intrinsics.copy(), p.group_model, p.cam_group, p.points[t:t + 1].copy(), p.obs_uv[sel],
                            p.obs_cam[sel], np.zeros(int(sel.sum()), np.int32), cam_const=np.full(p.cam_ext.shape[0], 3, np.uint8))


# ---------------------------------------------------------------- invalid observations
INVALID_MODEL = 5    # double sphere


def invalid_start_scene():
    """Part (a): the double-sphere scene with the w = -1 point, whose flipped q lies in the model's invalid region."""
    return edge_scene(INVALID_MODEL, 1, negative_w=True)


def invalid_candidate_scene(inside=0.005, beyond=0.1):
    """Part (b): a double-sphere scene valid at the start whose FIRST LM candidate is not.  One extra point stands two
    units beside camera 6, just inside the valid cone of that camera (z / |q| = -w2 + inside); cameras 0, 1 and 11, which
    see it in front of them, observe it beyond that cone (z / |q| = -w2 - beyond).  The first step follows those three
    observations, the candidate is invalid in camera 6, the step is rejected and the radius shrinks until the point stays
    inside (found with the oracle: five rejected steps, then an accepted one).  Returns (problem, index of the point, the
    position the three cameras pull it to)."""
    p = edge_scene(INVALID_MODEL, 1, perturb=0.2, negative_w=False)
    c = 6
    k = p.intrinsics[p.cam_group[c]]
    al, xi = k[6], k[5]
    w1 = (1.0 - al) / al if al > 0.5 else al / (1.0 - al)
    w2 = (w1 + xi) / np.sqrt(2.0 * w1 * xi + xi * xi + 1.0)
    R = angle_axis_to_matrix(p.cam_ext[c, 3:])

    def at(cosang, d=2.0):     # the world point at distance d from camera c whose q has z / |q| = cosang, in the camera's x-z plane
        q = d * np.array([np.sqrt(1.0 - cosang * cosang), 0.0, cosang])
        return p.cam_ext[c, :3] + R.T @ q
    X0, Xt = at(-w2 + inside), at(-w2 - beyond)
    cams = np.array([c, 0, 1, 11], np.int32)
    np_ = p.points.shape[0]
    q = capi.FlatProblem(p.cam_ext, p.intrinsics, p.group_model, p.cam_group, np.vstack([p.points, np.append(X0, 1.0)]),
                         np.zeros((len(p.obs_cam) + 4, 2)), np.concatenate([p.obs_cam, cams]),
                         np.concatenate([p.obs_pt, np.full(4, np_, np.int32)]))
    pts_t = q.points.copy(); pts_t[-1, :3] = Xt
    _, uv0 = project_with_oracle(q, q.cam_ext, q.points)     # camera 6: where the point stands at the start
    _, uvt = project_with_oracle(q, q.cam_ext, pts_t)        # the others: where the step will take it
    q.obs_uv[: len(p.obs_uv)] = p.obs_uv
    q.obs_uv[-4] = uv0[-4]
    q.obs_uv[-3:] = uvt[-3:]
    return q, np_, Xt
