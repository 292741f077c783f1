"""Small track sets for the triangulation stage of theia_hip_estimate_tracks and for theia_hip_track_statistics (test side only).

track_cut(model) is at most 48 tracks of tests/ba_edge_scenes.edge_scene(model) at its true state (perturb = 0: the cameras with the
zero and the 1e-9 angle-axis, three intrinsics groups with skew on both sides of 0 and aspect ratio on both sides of 1), observed
by the oracle's projection plus the scene's 0.5 px noise:

  * the planted points -- the world origin, w = 0.25, w = -1 where the model allows it, one on-axis point per group -- and the ten
    tracks cameras 0 and 1 have to themselves;
  * the first tracks of every length 2 .. 10 (for the fisheye model also the points behind cameras 5 and 8);
  * one 65-observation track (es.with_long_tracks), the last of them.

Observations of a point behind their camera are dropped (a pixel un-projects to a ray in front), the points handed to the device
are (0, 0, 0, 1), and `truth` keeps the true homogeneous points.  The viewing rays come from camera.ObservationRays on the device
(rays()); the tracks built by hand carry their own rays, exact to the bit, in `ray_override`.

The pinhole cut is followed by tracks built by hand on extra pinhole cameras of group 0 (`hand` names their indices):

  antiparallel   cameras at (0, 0, -5) and (0, 0, 5), rays (0, 0, 1) and (0, 0, -1): A = sum (I - d d^T) = diag(2, 2, 0) exactly, the
                 dot product is -1, so the angle test passes and the third pivot of the Cholesky is exactly 0: a failed
                 triangulation (Eigen's LLT reports a pivot <= 0).  The second camera is unrotated: the point is behind it.
  last_pair      six observations, five with the same ray, the sixth 10 degrees off;
  last_pair_only six observations whose ONLY pair above 3 degrees is the last one: four equal rays, then one 1.6 degrees to each side;
  above / below  two views at 3 degrees x (1 +- 1e-9): the dot products are 2.7e-12 to either side of cos(3 deg);
  one_view / no_view   one observation / none.

No track is known whose mu iteration does not settle (test_triangulation_ref.test_search_for_an_unsettled_track); one that is found
belongs here, next to these.

variant(model, name): "cut"; "far" (cameras and truth moved by (1e4, -2e4, 5e3): the cancellation in the midpoint's b = sum T o);
"interleaved" (the observation arrays permuted so that tracks interleave, each track's own observations in their order);
"double" (the cut followed by its far copy on cameras of its own, 2 x the tracks: the batches of 64 and 65 tracks, which a single
cut of at most 48 + 8 tracks does not reach, are cut from it)."""
import functools
import types

import numpy as np

from pytheiasfm_amd import _capi as capi
from tests import ba_edge_scenes as es

MODELS = tuple(range(8))
MAX_EDGE_TRACKS = 48
FAR = np.array([1e4, -2e4, 5e3])
MIN_ANGLE_DEG = 3.0
HAND_CAMERA_K = es.INTRINSICS[0][0]


def _depth(p, cam_ext, points):
    q = es.camera_frame(cam_ext, points, p.obs_cam, p.obs_pt)
    return q[:, 2] / points[p.obs_pt, 3]


def _rot_y(deg):
    a = np.deg2rad(deg)
    return np.array([np.sin(a), 0.0, np.cos(a)])      # (0, 0, 1) turned about y: a unit vector up to rounding


def _hand_tracks(nc0):
    """The tracks built by hand: (cameras [k][6], [(name, truth [3], [(camera, ray [3])])]).  A camera stands 6 away from its
    point against its ray and is turned by the ray's angle about y, so that the pixel is near the principal point."""
    cams, tracks = [], []

    def cam(pos, rot_deg=0.0):
        cams.append(np.concatenate([pos, [0.0, -np.deg2rad(rot_deg), 0.0]]))     # R^T e_z = (sin, 0, cos) of rot_deg
        return nc0 + len(cams) - 1

    def looking(X, deg):     # a camera 6 behind X along the ray at `deg`, turned the same way
        d = _rot_y(deg)
        return cam(X - 6.0 * d, deg), d

    a, b = cam([0.0, 0.0, -5.0]), cam([0.0, 0.0, 5.0])
    tracks.append(("antiparallel", np.zeros(3), [(a, np.array([0.0, 0.0, 1.0])), (b, np.array([0.0, 0.0, -1.0]))]))
    X = np.array([0.2, -0.1, 0.3])
    (c0, d0), (c1, d1) = looking(X, 0.0), looking(X, 10.0)
    tracks.append(("last_pair", X, [(c0, d0)] * 5 + [(c1, d1)]))
    X = np.array([-0.3, 0.2, 0.1])
    (c0, d0), (c1, d1), (c2, d2) = looking(X, 0.0), looking(X, 1.6), looking(X, -1.6)
    tracks.append(("last_pair_only", X, [(c0, d0)] * 4 + [(c1, d1), (c2, d2)]))
    X = np.array([0.1, 0.3, -0.2])
    c0, d0 = looking(X, 0.0)
    for name, sign in (("above", 1.0), ("below", -1.0)):
        c1, d1 = looking(X, MIN_ANGLE_DEG * (1.0 + sign * 1e-9))
        tracks.append((name, X, [(c0, d0), (c1, d1)]))
    tracks.append(("one_view", np.array([0.4, 0.1, 0.2]), [(a, None)]))
    tracks.append(("no_view", np.array([0.5, -0.4, 0.3]), []))
    return np.array(cams), tracks


def two_view_candidates(nseeds=400):
    """The inputs of the search for a track whose mu iteration does not settle: per seed one two-view pinhole track 3 .. 3.6 degrees
    apart with 8 .. 50 px noise on its pixels.  -> [(cams [2][6], rays [2][3], X [3], uv [2][2])]."""
    cams, Xs, rays, sig = [], [], [], []
    for seed in range(nseeds):
        rng = np.random.default_rng([0x5E77, seed])
        X = 1.6 * rng.random(3) - 0.8
        a0 = 20.0 * rng.random() - 10.0
        for a in (a0, a0 + MIN_ANGLE_DEG * (1.0 + 0.2 * rng.random())):
            d = _rot_y(a)
            cams.append(np.concatenate([X - (5.0 + 3.0 * rng.random()) * d, [0.0, -np.deg2rad(a), 0.0]])); rays.append(d)
        Xs.append(np.append(X, 1.0)); sig.append(8.0 + 42.0 * rng.random())
    n = len(Xs)
    k = np.zeros((1, capi.THEIA_MAX_INTRINSICS)); k[0, :len(HAND_CAMERA_K)] = HAND_CAMERA_K
    p = capi.FlatProblem(np.array(cams), k, [0], np.zeros(2 * n, np.int32), np.array(Xs), np.zeros((2 * n, 2)), np.arange(2 * n, dtype=np.int32),
                         np.repeat(np.arange(n, dtype=np.int32), 2))
    ok, uv = es.project_with_oracle(p, p.cam_ext, p.points)
    assert ok == 1
    out = []
    for s in range(n):
        rng = np.random.default_rng([0x5E78, s])
        out.append((p.cam_ext[2 * s:2 * s + 2].copy(), np.array(rays[2 * s:2 * s + 2]), p.points[s, :3].copy(),
                    uv[2 * s:2 * s + 2] + sig[s] * rng.standard_normal((2, 2))))
    return out


def _select(p, model, info):
    """The tracks of the edge scene that go into the cut, in their order, the long track last."""
    npts = p.points.shape[0] - 1                  # (the last point is the 65-observation track)
    planted = [0, 1] + ([2] if model in es.NEGATIVE_W_MODELS else [])
    axis = info["axis"][0::3]
    pair01 = [t for t in range(npts) if set(p.obs_cam[p.obs_pt == t].tolist()) == {0, 1}]
    chosen = planted + axis + pair01
    if model == 2:
        chosen += [npts - 4, npts - 3]               # behind camera 5 / camera 8
    for t in range(info["planted"], npts):
        if len(chosen) >= MAX_EDGE_TRACKS - 1:
            break
        if t not in chosen:
            chosen.append(t)
    return sorted(chosen) + [npts], {"origin": 0, "w_quarter": 1, "w_negative": 2 if model in es.NEGATIVE_W_MODELS else None,
                                     "axis": axis, "pair01": pair01, "long": npts}


def _sub(p, tracks, points=None):
    """p restricted to `tracks` (renumbered in that order), every camera kept."""
    new = np.full(p.points.shape[0], -1, np.int64); new[np.asarray(tracks)] = np.arange(len(tracks))
    keep = new[p.obs_pt] >= 0
    order = np.flatnonzero(keep)
    order = order[np.argsort(new[p.obs_pt[order]], kind="stable")]
    pc = None if p.point_const is None else p.point_const[np.asarray(tracks)]
    q = capi.FlatProblem(p.cam_ext, p.intrinsics, p.group_model, p.cam_group, (p.points if points is None else points)[np.asarray(tracks)],
                         p.obs_uv[order], p.obs_cam[order], new[p.obs_pt[order]].astype(np.int32), point_const=pc)
    return q, order


@functools.lru_cache(maxsize=None)
def track_cut(model):
    model = int(model)
    base = es._edge_scene((model,) * 3, 1, 0.0, model in es.NEGATIVE_W_MODELS)
    p = es.with_long_tracks(base[0].copy(), nlong=1, nobs=65)
    tracks, names = _select(p, model, base[1])
    front = _depth(p, p.cam_ext, p.points) > 0.0
    fp = capi.FlatProblem(p.cam_ext, p.intrinsics, p.group_model, p.cam_group, p.points, p.obs_uv[front], p.obs_cam[front], p.obs_pt[front])
    q, _ = _sub(fp, tracks)
    names = {k: (None if v is None else [tracks.index(t) for t in v] if isinstance(v, list) else tracks.index(v)) for k, v in names.items()}
    truth = q.points.copy()
    hand, override = {}, {}
    if model == 0:
        nc0, np0, no0 = q.cam_ext.shape[0], q.points.shape[0], q.obs_uv.shape[0]
        cams, built = _hand_tracks(nc0)
        oc, op, rays, pts = [], [], [], []
        for name, X, obs in built:
            hand[name] = np0 + len(pts)
            for c, d in obs:
                oc.append(c); op.append(hand[name]); rays.append(d)
            pts.append(np.append(X, 1.0))
        cam_ext = np.vstack([q.cam_ext, cams])
        truth = np.vstack([truth, pts])
        group = np.concatenate([q.cam_group, np.zeros(len(cams), np.int32)])
        full = capi.FlatProblem(cam_ext, q.intrinsics, q.group_model, group, truth.copy(), np.zeros((no0 + len(oc), 2)),
                                np.concatenate([q.obs_cam, np.asarray(oc, np.int32)]), np.concatenate([q.obs_pt, np.asarray(op, np.int32)]))
        ok, uv = es.project_with_oracle(full, full.cam_ext, full.points)     # the hand-built pixels: where the point projects, no noise
        assert ok == 1
        full.obs_uv[:no0] = q.obs_uv
        full.obs_uv[no0:] = uv[no0:]
        override = {no0 + i: d for i, d in enumerate(rays) if d is not None}
        q = full
    q.points[:] = [0.0, 0.0, 0.0, 1.0]
    return types.SimpleNamespace(model=model, p=q, truth=truth, names=names, hand=hand, ray_override=override, parent=None)


@functools.lru_cache(maxsize=None)
def variant(model, name="cut"):
    cut = track_cut(model)
    if name == "cut":
        return cut
    p = cut.p
    if name == "far":
        q = p.copy()
        q.cam_ext[:, :3] += FAR
        truth = cut.truth.copy(); truth[:, :3] += truth[:, 3:4] * FAR
        return types.SimpleNamespace(model=cut.model, p=q, truth=truth, names=cut.names, hand=cut.hand, ray_override=cut.ray_override, parent=None)
    if name == "interleaved":
        rank = np.zeros(len(p.obs_pt), np.int64)
        seen = {}
        for i, t in enumerate(p.obs_pt.tolist()):
            rank[i] = seen.get(t, 0); seen[t] = rank[i] + 1
        perm = np.lexsort((p.obs_pt, rank))          # round-robin over the tracks; within a track the ranks ascend
        q = capi.FlatProblem(p.cam_ext, p.intrinsics, p.group_model, p.cam_group, p.points, p.obs_uv[perm], p.obs_cam[perm], p.obs_pt[perm])
        return types.SimpleNamespace(model=cut.model, p=q, truth=cut.truth, names=cut.names, hand=cut.hand,
                                     ray_override={int(np.flatnonzero(perm == i)[0]): d for i, d in cut.ray_override.items()}, parent=perm)
    if name == "double":
        far = variant(model, "far")
        nc, npts, no = p.cam_ext.shape[0], p.points.shape[0], p.obs_uv.shape[0]
        q = capi.FlatProblem(np.vstack([p.cam_ext, far.p.cam_ext]), p.intrinsics, p.group_model, np.concatenate([p.cam_group, p.cam_group]),
                             np.vstack([p.points, p.points]), np.vstack([p.obs_uv, p.obs_uv]), np.concatenate([p.obs_cam, p.obs_cam + nc]),
                             np.concatenate([p.obs_pt, p.obs_pt + npts]))
        over = dict(cut.ray_override); over.update({i + no: d for i, d in cut.ray_override.items()})
        return types.SimpleNamespace(model=cut.model, p=q, truth=np.vstack([cut.truth, far.truth]), names=cut.names, hand=cut.hand,
                                     ray_override=over, parent=np.concatenate([np.arange(no), np.arange(no)]))
    raise KeyError(name)


def first_tracks(cutv, n):
    """The first n tracks of a variant as a problem of their own, and the rows of the variant's observations they keep."""
    return _sub(cutv.p, list(range(n)))


def with_truth(cutv):
    """The variant's problem at its true points (the state of the statistics tests)."""
    q = cutv.p.copy()
    q.points[:] = cutv.truth
    return q


def numpy_rays(cutv):
    """Unit rays from the camera centres at the true points (no device: the CPU tests' stand-in for rays()), with the hand-built ones."""
    p = cutv.p
    X = cutv.truth[p.obs_pt]
    d = X[:, :3] / X[:, 3:4] - p.cam_ext[p.obs_cam, :3]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    for i, v in cutv.ray_override.items():
        d[i] = v
    return d


def rays(cutv):
    """camera.ObservationRays of the variant (a device call), the hand-built rays put in their rows bit for bit."""
    from pytheiasfm_amd import camera
    d = np.array(camera.ObservationRays(cutv.p))
    for i, v in cutv.ray_override.items():
        d[i] = v
    return np.ascontiguousarray(d)
