"""Co-visibility on the device (csrc/covisibility.hip; include/theia_hip.h has the rules, the deviations and the
refusals): the view graph of a reconstruction, the MVSNet view selection, and the tracks common to a set of views.

Array level: covisibility_graph, mvsnet_pair_scores, view_selection_mvsnet, find_common_tracks.
pyTheia's names over the mirror's Reconstruction (sfm.Reconstruction: ids are dense indices):
ViewGraphFromReconstruction, ViewSelectionMVSNet, FindCommonTracksInViews."""
import ctypes as C

import numpy as np

from . import _capi as capi
from .twoview import TwoViewInfo

DEFAULT_WINDOW = 8192   # THEIA_COVISIBILITY_DEFAULT_WINDOW


def _refuse(text):
    return capi.TheiaHipError(capi.THEIA_HIP_ERR_INVALID_ARGUMENT, text)


def _observations(obs_view, obs_track):
    ov = np.ascontiguousarray(np.asarray(obs_view, dtype=np.int32).reshape(-1))
    ot = np.ascontiguousarray(np.asarray(obs_track, dtype=np.int32).reshape(-1))
    if ov.shape != ot.shape:
        raise _refuse("obs_view and obs_track differ in length")
    return ov, ot


def _flags(flags, n, what):
    if flags is None:
        return None
    f = np.ascontiguousarray(np.asarray(flags, dtype=bool).reshape(-1).astype(np.uint8))
    if f.shape != (n,):
        raise _refuse(f"{what} must have one entry per item")
    return f


def _rows(a, n, width, what):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1, width))
    if a.shape[0] != n:
        raise _refuse(f"{what} must be [{n}][{width}]")
    return a


def covisibility_graph(num_views, num_tracks, obs_view, obs_track, view_estimated=None, track_estimated=None, cam_ext=None,
                       min_shared_tracks=0, column_window=0):
    """theia_hip_covisibility_graph on arrays.  Returns (pairs [E][2] int32 ascending in (i, j), num_shared [E] int32,
    rotation_2 [E][3], position_2 [E][3]); the last two are None without cam_ext."""
    ov, ot = _observations(obs_view, obs_track)
    nv, nt = int(num_views), int(num_tracks)
    ve, te = _flags(view_estimated, nv, "view_estimated"), _flags(track_estimated, nt, "track_estimated")
    cam = None if cam_ext is None else _rows(cam_ext, nv, 6, "cam_ext")
    L = capi.lib()
    count = C.c_int64(0)

    def call(capacity):
        pairs = np.zeros((capacity, 2), np.int32); shared = np.zeros(capacity, np.int32)
        rot = None if cam is None else np.zeros((capacity, 3)); pos = None if cam is None else np.zeros((capacity, 3))
        capi.check(L.theia_hip_covisibility_graph(nv, nt, len(ov), capi.ptr(ov, C.c_int32), capi.ptr(ot, C.c_int32),
                                                  capi.ptr(ve, C.c_uint8), capi.ptr(te, C.c_uint8), capi.ptr(cam, C.c_double),
                                                  int(min_shared_tracks), int(column_window), capacity,
                                                  capi.ptr(pairs, C.c_int32), capi.ptr(shared, C.c_int32),
                                                  capi.ptr(rot, C.c_double), capi.ptr(pos, C.c_double), C.byref(count)))
        return pairs, shared, rot, pos

    # a guess of 64 neighbours per view (never more than all pairs); a larger count repeats the call with it
    capacity = max(0, min(nv * (nv - 1) // 2, 64 * nv))
    out = call(capacity)
    if count.value > capacity:
        out = call(count.value)
    E = count.value
    return tuple(None if a is None else a[:E] for a in out)


def mvsnet_pair_scores(num_views, num_tracks, obs_view, obs_track, cam_ext, points, pairs, theta0, sigma1, sigma2,
                       track_mask=None):
    """theia_hip_mvsnet_pair_scores on arrays: (score [E] float64, num_common [E] int32) for pairs [E][2]."""
    ov, ot = _observations(obs_view, obs_track)
    nv, nt = int(num_views), int(num_tracks)
    cam, pts = _rows(cam_ext, nv, 6, "cam_ext"), _rows(points, nt, 4, "points")
    mask = _flags(track_mask, nt, "track_mask")
    p = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
    score = np.zeros(len(p)); common = np.zeros(len(p), np.int32)
    capi.check(capi.lib().theia_hip_mvsnet_pair_scores(
        nv, nt, len(ov), capi.ptr(ov, C.c_int32), capi.ptr(ot, C.c_int32), capi.ptr(cam, C.c_double), capi.ptr(pts, C.c_double),
        capi.ptr(mask, C.c_uint8), len(p), capi.ptr(p, C.c_int32), float(theta0), float(sigma1), float(sigma2),
        capi.ptr(score, C.c_double), capi.ptr(common, C.c_int32)))
    return score, common


def view_selection_mvsnet(num_views, num_tracks, obs_view, obs_track, view_estimated, track_estimated, cam_ext, points,
                          num_neighbors, theta0, sigma1, sigma2, min_shared_tracks=10, column_window=0):
    """theia_hip_view_selection_mvsnet on arrays: (neighbor [V][k] int32, -1 padded; score [V][k]), best first."""
    ov, ot = _observations(obs_view, obs_track)
    nv, nt, k = int(num_views), int(num_tracks), int(num_neighbors)
    ve, te = _flags(view_estimated, nv, "view_estimated"), _flags(track_estimated, nt, "track_estimated")
    cam, pts = _rows(cam_ext, nv, 6, "cam_ext"), _rows(points, nt, 4, "points")
    neighbor = np.full((max(nv, 0), max(k, 0)), -1, np.int32); score = np.zeros((max(nv, 0), max(k, 0)))
    capi.check(capi.lib().theia_hip_view_selection_mvsnet(
        nv, nt, len(ov), capi.ptr(ov, C.c_int32), capi.ptr(ot, C.c_int32), capi.ptr(ve, C.c_uint8), capi.ptr(te, C.c_uint8),
        capi.ptr(cam, C.c_double), capi.ptr(pts, C.c_double), int(min_shared_tracks), k, float(theta0), float(sigma1),
        float(sigma2), int(column_window), capi.ptr(neighbor, C.c_int32), capi.ptr(score, C.c_double)))
    return neighbor, score


def find_common_tracks(num_views, num_tracks, obs_view, obs_track, queries):
    """theia_hip_find_common_tracks for a list of queries, each a sequence of at least two views: a list of int32 arrays,
    every one the ascending tracks all views of its query observe."""
    ov, ot = _observations(obs_view, obs_track)
    lists = [np.asarray(list(q), dtype=np.int32).reshape(-1) for q in queries]
    Q = len(lists)
    if Q == 0:
        return []
    offsets = np.zeros(Q + 1, np.int64)
    offsets[1:] = np.cumsum([len(q) for q in lists])
    views = np.ascontiguousarray(np.concatenate(lists).astype(np.int32))
    track_off = np.zeros(Q + 1, np.int64)
    found = C.c_int64(0)
    L = capi.lib()

    def call(capacity):
        tracks = np.zeros(capacity, np.int32)
        capi.check(L.theia_hip_find_common_tracks(int(num_views), int(num_tracks), len(ov), capi.ptr(ov, C.c_int32),
                                                  capi.ptr(ot, C.c_int32), Q, capi.ptr(offsets, C.c_int64),
                                                  capi.ptr(views, C.c_int32), capacity, capi.ptr(track_off, C.c_int64),
                                                  capi.ptr(tracks, C.c_int32), C.byref(found)))
        return tracks

    # no answer is longer than its shortest list, and none longer than the observations
    capacity = min(len(ov) * Q, 1 << 20)
    tracks = call(capacity)
    if found.value > capacity:
        tracks = call(found.value)
    return [tracks[track_off[q]:track_off[q + 1]].copy() for q in range(Q)]


# ------------------------------------------------------------------------------------------------- pyTheia's names

def ViewGraphFromReconstruction(reconstruction, min_shared_tracks, column_window=0):
    """ViewGraphFromReconstruction(reconstruction, min_shared_tracks, &view_graph) with the {(id1, id2): TwoViewInfo} dict
    that stands in for the ViewGraph (global_pose.py's estimators and filters take it): id1 < id2, in ascending order."""
    r = reconstruction
    pairs, shared, rot, pos = covisibility_graph(r.NumViews(), r.NumTracks(), r.obs_view, r.obs_track, r.view_estimated,
                                                 r.track_estimated, r.cam_ext, min_shared_tracks, column_window)
    view_pairs = {}
    for (a, b), n, w, p in zip(pairs.tolist(), shared.tolist(), rot, pos):
        info = TwoViewInfo()
        info.rotation_2 = w.copy()
        info.position_2 = p.copy()
        info.num_verified_matches = int(n)
        view_pairs[(a, b)] = info
    return view_pairs


def ViewSelectionMVSNet(reconstruction, num_neighbors, theta0, sigma1, sigma2):
    """ViewSelectionMVSNet(reconstruction, num_neighbors, theta0, sigma1, sigma2) (pybind mvs.cc:44): {view: [(score,
    neighbour), ...]} for every estimated view, best first (the reference's map iterates in descending score)."""
    r = reconstruction
    neighbor, score = view_selection_mvsnet(r.NumViews(), r.NumTracks(), r.obs_view, r.obs_track, r.view_estimated,
                                            r.track_estimated, r.cam_ext, r.points, num_neighbors, theta0, sigma1, sigma2)
    est = np.asarray(r.view_estimated, dtype=bool)
    return {v: [(float(s), int(n)) for s, n in zip(score[v], neighbor[v]) if n >= 0] for v in range(r.NumViews()) if est[v]}


def FindCommonTracksInViews(reconstruction, views):
    """FindCommonTracksInViews(reconstruction, views) (pybind sfm.cc:939): the ascending list of the tracks every one of
    the views observes."""
    r = reconstruction
    return find_common_tracks(r.NumViews(), r.NumTracks(), r.obs_view, r.obs_track, [views])[0].tolist()
