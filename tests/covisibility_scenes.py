"""Seeded scenes of tests/test_covisibility.py and tests/test_covisibility_gpu.py.  A scene is a dict of the arrays the
co-visibility entries read: num_views, num_tracks, obs_view, obs_track (shuffled rows), view_estimated, track_estimated,
cam_ext [V][6] = position | angle-axis, points [T][4] homogeneous with w != 1."""
import numpy as np

from pytheiasfm_amd import sfm

THETA0, SIGMA1, SIGMA2 = 5.0, 1.0, 10.0   # the values pyTheia's examples call ViewSelectionMVSNet with


def _look_free_orientations(rng, n):
    w = rng.standard_normal((n, 3))
    return w / np.linalg.norm(w, axis=1, keepdims=True) * rng.uniform(0.2, 2.5, (n, 1))


def ring_scene(num_views=24, num_tracks=600, seed=7, min_len=3, max_len=8):
    """Views on a ring of radius 10 with z uniform in +-1, points uniform in +-3, every track seen by min_len .. max_len
    consecutive views (the ring wraps).  Everything estimated."""
    rng = np.random.default_rng(seed)
    ang = 2.0 * np.pi * np.arange(num_views) / num_views
    centres = np.stack([10.0 * np.cos(ang), 10.0 * np.sin(ang), rng.uniform(-1.0, 1.0, num_views)], axis=1)
    cam_ext = np.hstack([centres, _look_free_orientations(rng, num_views)])
    w = rng.uniform(0.5, 2.0, (num_tracks, 1))
    points = np.hstack([rng.uniform(-3.0, 3.0, (num_tracks, 3)) * w, w])
    first = rng.integers(0, num_views, num_tracks)
    length = rng.integers(min_len, max_len + 1, num_tracks)
    obs_view = np.concatenate([(f + np.arange(l)) % num_views for f, l in zip(first, length)]).astype(np.int32)
    obs_track = np.concatenate([np.full(l, t) for t, l in enumerate(length)]).astype(np.int32)
    order = rng.permutation(len(obs_view))
    return dict(num_views=num_views, num_tracks=num_tracks, obs_view=obs_view[order], obs_track=obs_track[order],
                view_estimated=np.ones(num_views, bool), track_estimated=np.ones(num_tracks, bool), cam_ext=cam_ext,
                points=points)


_cache = {}


def base_scene():
    if "base" not in _cache:
        _cache["base"] = ring_scene()
    return _cache["base"]


def variant_scene():
    """40 views, 900 tracks of 3 .. 12 consecutive views; views 13 and 29 observe nothing; every fifth view from 2 and every
    seventh track from 3 are unestimated; track 0 is a hub seen by every view that observes anything (38 of the 40)."""
    if "variant" not in _cache:
        s = ring_scene(40, 900, seed=11, max_len=12)
        empty = (13, 29)
        keep = ~np.isin(s["obs_view"], empty) & (s["obs_track"] != 0)
        hub = np.array([v for v in range(40) if v not in empty], dtype=np.int32)
        obs_view = np.concatenate([s["obs_view"][keep], hub]).astype(np.int32)
        obs_track = np.concatenate([s["obs_track"][keep], np.zeros(len(hub), np.int32)]).astype(np.int32)
        order = np.random.default_rng(12).permutation(len(obs_view))
        s["obs_view"], s["obs_track"] = obs_view[order], obs_track[order]
        s["view_estimated"] = np.arange(40) % 5 != 2
        s["track_estimated"] = np.arange(900) % 7 != 3
        _cache["variant"] = s
    return _cache["variant"]


def mirrored_scene():
    """Five views: view 0 on the plane x = 0, views 1 and 2 mirror images of each other in that plane, 16 points on it, all
    seen by views 0, 1 and 2; views 3 and 4 see nothing.  For a point on the plane the x coordinate of view 1 or 2 enters
    a term only as (+-2)^2 and as a product with view 0's zero, so score(0, 1) == score(0, 2) bit for bit, term by term."""
    n = 16
    rng = np.random.default_rng(5)
    pts = np.zeros((n, 4))
    pts[:, 1] = rng.uniform(4.0, 8.0, n); pts[:, 2] = rng.uniform(-2.0, 2.0, n); pts[:, 3] = 1.0
    cam_ext = np.zeros((5, 6))
    cam_ext[0, :3] = (0.0, -6.0, 0.5)
    cam_ext[1, :3] = (2.0, -5.0, 0.25)
    cam_ext[2, :3] = (-2.0, -5.0, 0.25)
    cam_ext[3, :3] = (9.0, 9.0, 9.0); cam_ext[4, :3] = (-9.0, 9.0, 9.0)
    obs_view = np.repeat(np.arange(3), n).astype(np.int32)
    obs_track = np.tile(np.arange(n), 3).astype(np.int32)
    return dict(num_views=5, num_tracks=n, obs_view=obs_view, obs_track=obs_track, view_estimated=np.ones(5, bool),
                track_estimated=np.ones(n, bool), cam_ext=cam_ext, points=pts)


def reconstruction(scene):
    """the scene as the mirror's Reconstruction"""
    r = sfm.Reconstruction()
    r.cam_ext = scene["cam_ext"].copy(); r.view_estimated = scene["view_estimated"].copy()
    r.points = scene["points"].copy(); r.track_estimated = scene["track_estimated"].copy()
    r.obs_view = scene["obs_view"].copy(); r.obs_track = scene["obs_track"].copy()
    return r


def common_track_queries(scene, count=50, seed=3):
    """`count` queries of 2 .. 6 views: neighbouring views mostly; query 0 has no common track (opposite sides of the ring),
    query 1 names a view twice."""
    rng = np.random.default_rng(seed)
    V = scene["num_views"]
    queries = [[0, V // 2], [5, 6, 5]]
    while len(queries) < count:
        k = int(rng.integers(2, 7))
        start = int(rng.integers(0, V))
        queries.append([(start + int(d)) % V for d in rng.permutation(k + 1)[:k]])
    return queries
