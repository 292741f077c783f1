"""Inverse-depth scenes for the tests: a synth_ba_v1 problem re-expressed in the reference's inverse-depth
parametrisation -- reference view = first observing view of a track, bearing = the reference camera's normalised ray
(x, y, 1) of the (noisy) feature as Reconstruction::... sets it (estimate_track.cc:281: PixelToNormalizedCoordinates),
inverse depth = 1 / depth in that view (bundle_adjustment.cc:67-83 UpdateInverseDepth)."""
import numpy as np

from pytheiasfm_amd import synth


def aa_to_rot(w):
    th = np.linalg.norm(w)
    if th < 1e-12:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def make(num_views=8, num_tracks=200, seed=5, rho_noise=0.02):
    """Returns a FlatProblem with set_inverse_depth() applied (pinhole groups only)."""
    p = synth.synth_ba_v1(num_views, num_tracks, seed=seed)
    nt = p.points.shape[0]
    order = np.argsort(p.obs_pt, kind="stable")
    first = np.full(nt, -1, dtype=np.int64)
    tr, idx = np.unique(p.obs_pt[order], return_index=True)
    first[tr] = order[idx]                       # first observation of every track
    ref_cam = p.obs_cam[first].astype(np.int32)
    bearing = np.zeros((nt, 3)); rho = np.zeros(nt)
    rng = np.random.default_rng(seed)
    for t in range(nt):
        c = ref_cam[t]
        f, a, s, px, py = p.intrinsics[p.cam_group[c]][:5]
        u, v = p.obs_uv[first[t]]
        y = (v - py) / (f * a); x = (u - px - s * y) / f
        bearing[t] = (x, y, 1.0)
        X = p.points[t, :3] / p.points[t, 3]
        depth = (aa_to_rot(p.cam_ext[c, 3:]) @ (X - p.cam_ext[c, :3]))[2]
        rho[t] = (1.0 / depth) * (1.0 + rho_noise * rng.normal())
    p.set_inverse_depth(ref_cam, bearing, rho)
    return p


def subset(p, keep):
    """p with the observations of the boolean mask `keep` only (every other array, the inverse-depth state included, as
    it is; fresh copies of what a solve changes)."""
    from pytheiasfm_amd import _capi as capi
    keep = np.asarray(keep, dtype=bool)
    q = capi.FlatProblem(p.cam_ext.copy(), p.intrinsics.copy(), p.group_model, p.cam_group, p.points.copy(), p.obs_uv[keep],
                         p.obs_cam[keep], p.obs_pt[keep], p.cam_const, p.group_const, p.point_const,
                         None if p.obs_sqrt_info is None else p.obs_sqrt_info[keep], p.flags)
    if p.point_ref_cam is not None:
        q.set_inverse_depth(p.point_ref_cam, p.point_ref_bearing, p.point_inverse_depth.copy())
    return q


def from_problem(p, reference="first", min_depth=0.5):
    """Any FlatProblem (any camera model) in inverse-depth form.  The reference view of a track is one of its observers that
    has the point at a depth > min_depth in the START state: the first / the last of them in observation order, or
    ("highest") the one with the largest camera index -- its block then lies below the observers' in the reduced system;
    "non_observer" is "first" with the reference view's own observation dropped afterwards.  The bearing is the start
    state's camera-frame point over its z (no model is unprojected) and rho = 1 / z.  Constant masks, groups, sqrt
    information and observations are p's."""
    from tests import ba_edge_scenes as es
    assert reference in ("first", "last", "highest", "non_observer")
    nt = p.points.shape[0]
    q = es.camera_frame(p.cam_ext, p.points, p.obs_cam, p.obs_pt) / p.points[p.obs_pt, 3:4]   # the point itself, not w times it
    ref_obs = np.full(nt, -1, dtype=np.int64)
    for i in range(len(p.obs_pt)):
        t = p.obs_pt[i]
        if not q[i, 2] > min_depth:
            continue
        if ref_obs[t] < 0 or reference == "last" or (reference == "highest" and p.obs_cam[i] > p.obs_cam[ref_obs[t]]):
            ref_obs[t] = i
    assert (ref_obs >= 0).all(), "every track needs an observer that has it in front"
    bearing = q[ref_obs] / q[ref_obs, 2:3]
    out = subset(p, np.ones(len(p.obs_pt), dtype=bool))
    out.set_inverse_depth(p.obs_cam[ref_obs], bearing, 1.0 / q[ref_obs, 2])
    if reference == "non_observer":
        keep = np.ones(len(p.obs_pt), dtype=bool); keep[ref_obs] = False
        out = subset(out, keep)
    return out


def without_reference_observation(p, tracks):
    """p without the observations the listed tracks have in their own reference view."""
    drop = np.isin(p.obs_pt, tracks) & (p.obs_cam == p.point_ref_cam[p.obs_pt])
    return subset(p, ~drop)


def cut_to_reference(p, tracks):
    """p with the listed tracks cut down to the observation in their reference view."""
    drop = np.isin(p.obs_pt, tracks) & (p.obs_cam != p.point_ref_cam[p.obs_pt])
    return subset(p, ~drop)


def reference_only(p):
    """Mask of the tracks seen by their reference view alone (the projection of b / rho does not depend on rho in a central
    model: their rho is unobservable)."""
    nt = p.points.shape[0]
    same = p.obs_cam == p.point_ref_cam[p.obs_pt]
    return (np.bincount(p.obs_pt, minlength=nt) > 0) & (np.bincount(p.obs_pt[~same], minlength=nt) == 0)


def _excess(a, b, rtol, atol):
    """max |a - b| / (atol + rtol |b|): np.allclose(a, b, rtol, atol) is `excess <= 1` (a NaN fails either)."""
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    if a.size == 0:
        return 0.0
    return float((np.abs(a - b) / (atol + rtol * np.abs(b))).max())


def compare(g, o, scale=1.0, skip_rho=None, step_norm=False, label=None):
    """Two solves (problem, summary, trace) of one inverse-depth problem against each other: the same accept list, the LM
    trace (cost rtol 1e-9, gradient max norm rtol 1e-6), cameras and rho to 1e-8, intrinsics rtol 1e-9.  The device is held
    to these with scale = 1; two runs of the oracle on inputs 1e-15 apart to a tenth of them (scale = 0.1) before a
    case is used.  skip_rho: mask of the tracks whose rho is left out (unobservable ones).  step_norm: the trace's step
    norms as well -- linear in the gradient, so at its rtol 1e-6, with the parameters' 1e-8 as the absolute floor.
    Returns the deviations in units of their tolerance; with a label it prints them and the raw figures."""
    (qg, sg, tg), (qo, so, to) = g, o
    assert sg.success and so.success and sg.num_iterations == so.num_iterations
    assert list(tg.accepted) == list(to.accepted)
    # (the device sums with FP64 atomics: a gradient eight orders below its start carries their rounding, run to run)
    keep = np.ones(len(qo.point_inverse_depth), dtype=bool) if skip_rho is None else ~np.asarray(skip_rho, dtype=bool)
    d_cam = float(np.abs(qg.cam_ext - qo.cam_ext).max())
    d_rho = float(np.abs(qg.point_inverse_depth - qo.point_inverse_depth)[keep].max()) if keep.any() else 0.0
    dev = {"cost": _excess(tg.cost, to.cost, 1e-9, 1e-8),
           "gradient": _excess(tg.gradient_max_norm, to.gradient_max_norm, 1e-6, 1e-9 * max(1.0, float(to.gradient_max_norm[0]))),
           "cam_ext": d_cam / 1e-8, "rho": d_rho / 1e-8,
           "intrinsics": _excess(qg.intrinsics, qo.intrinsics, 1e-9, 1e-12)}
    if step_norm:
        dev["step_norm"] = _excess(tg.step_norm, to.step_norm, 1e-6, 1e-8)
    if label is not None:
        rel = lambda a, b: float((np.abs(np.asarray(a) - np.asarray(b)) / np.maximum(np.abs(b), 1e-300)).max())
        print("%s: %d iterations, accepted %s | cost rel %.2e, gradient rel %.2e, cam_ext abs %.2e, rho abs %.2e, intrinsics abs %.2e | "
              "in units of the tolerance: %s" % (label, so.num_iterations, "".join(str(int(a)) for a in to.accepted), rel(tg.cost, to.cost),
                                                 rel(tg.gradient_max_norm, to.gradient_max_norm), d_cam, d_rho,
                                                 float(np.abs(qg.intrinsics - qo.intrinsics).max()),
                                                 ", ".join("%s %.3g" % kv for kv in dev.items())))
    for name, v in dev.items():
        assert v <= scale, (label, name, v, scale)
    return dev


def world_points(p):
    """UpdateHomogeneousPoint (bundle_adjustment.cc:47-65): X = R_ref^T (b / rho) + c_ref."""
    out = np.ones((p.points.shape[0], 4))
    for t in range(p.points.shape[0]):
        c = p.point_ref_cam[t]
        out[t, :3] = aa_to_rot(p.cam_ext[c, 3:]).T @ (p.point_ref_bearing[t] / p.point_inverse_depth[t]) + p.cam_ext[c, :3]
    return out
