"""Synthetic scenes of the LiGT position tests, in the set-up of the reference's own test: camera positions
10 U(-1, 1)^3, orientations (angle-axis) 0.2 U(-1, 1)^3, points U(-1, 1)^3 + (0, 0, 20); a track sees `obs_per_track`
distinct views in a random order; the feature is hnormalized(R (X - c)), plus Gaussian noise when asked.  The view pairs
(for the sign vote) are a ring over the views plus as many random pairs, with position_2 = R_i (c_j - c_i) / |.|.

The sizes are the smallest that reach each path of csrc/ligt_positions.hip: 6 views (one 64-tile), 20 views, 70 views
(n = 207: four 64-tiles, the last ragged); extra tracks of 2 observations (skipped), exactly 3, all 20 views (190 pairs:
the pair loop runs past one wave) and all 70 views (2 415 pairs); two views that no used track names."""
import numpy as np

from tests import ligt_positions_ref as ref


def make_scene(num_views, num_tracks, obs_per_track, seed, noise=0.0, extra_tracks=(), unused_views=0):
    """extra_tracks: lengths of tracks appended after the regular ones (a length of num_views sees every view).
    unused_views: that many additional views, appended, which only tracks of 2 observations name."""
    rng = np.random.default_rng(seed)
    nv = num_views + unused_views
    pos = 10.0 * rng.uniform(-1, 1, (nv, 3))
    aa = 0.2 * rng.uniform(-1, 1, (nv, 3))
    R = np.array([ref.rotation_matrix(w) for w in aa])
    lengths = [obs_per_track] * num_tracks + list(extra_tracks)
    pts = rng.uniform(-1, 1, (len(lengths), 3)) + np.array([0.0, 0.0, 20.0])
    obs_view, obs_feat, offsets = [], [], [0]
    for t, L in enumerate(lengths):
        views = rng.permutation(num_views)[:L]
        for v in views:
            p = R[v] @ (pts[t] - pos[v])
            obs_view.append(v)
            obs_feat.append(p[:2] / p[2])
        offsets.append(len(obs_view))
    for u in range(unused_views):   # a 2-observation track each: named, never used
        v = num_views + u
        for w in (v, int(rng.integers(num_views))):
            p = R[w] @ (pts[0] - pos[w])
            obs_view.append(w)
            obs_feat.append(p[:2] / p[2])
        offsets.append(len(obs_view))
    obs_feat = np.array(obs_feat)
    if noise > 0.0:
        obs_feat = obs_feat + noise * rng.standard_normal(obs_feat.shape)
    ring = [(i, (i + 1) % nv) for i in range(nv)]
    rand = [tuple(rng.permutation(nv)[:2]) for _ in range(nv)]
    edges = np.array(ring + rand, dtype=np.int32)
    rel = np.array([R[i] @ (pos[j] - pos[i]) / np.linalg.norm(pos[j] - pos[i]) for i, j in edges])
    return dict(orientations=aa, positions=pos, track_offsets=np.array(offsets, dtype=np.int32),
                obs_view=np.array(obs_view, dtype=np.int32), obs_feature=obs_feat, edges=edges, rel=rel,
                num_views=nv, noise=noise)


# name -> make_scene arguments.  The seeds are checked by test_ligt_positions.py: on every scene the best and second-best
# theta^2 of every used track differ by more than 1e-9 relative.
SCENES = {
    "v6": dict(num_views=6, num_tracks=40, obs_per_track=4, seed=11),
    "v20": dict(num_views=20, num_tracks=200, obs_per_track=5, seed=12),
    "v70": dict(num_views=70, num_tracks=600, obs_per_track=6, seed=13),
    "v20_extra": dict(num_views=20, num_tracks=200, obs_per_track=5, seed=12, extra_tracks=(2, 3, 20)),
    "v70_long": dict(num_views=70, num_tracks=600, obs_per_track=6, seed=13, extra_tracks=(70,)),
    "v20_unused": dict(num_views=20, num_tracks=200, obs_per_track=5, seed=14, unused_views=2),
    "v6_noisy": dict(num_views=6, num_tracks=40, obs_per_track=4, seed=11, noise=1e-3),
    "v20_noisy": dict(num_views=20, num_tracks=200, obs_per_track=5, seed=12, noise=1e-3),
    "v70_noisy": dict(num_views=70, num_tracks=600, obs_per_track=6, seed=13, noise=1e-3),
}
NOISE_FREE = ("v6", "v20", "v70")
NOISY = ("v6_noisy", "v20_noisy", "v70_noisy")

_cache = {}


def scene(name):
    """The scene and its reference solution, computed once and shared: (scene dict, ligt_positions_ref.estimate dict).
    Neither is to be modified."""
    if name not in _cache:
        s = make_scene(**SCENES[name])
        r = ref.estimate(s["orientations"], s["track_offsets"], s["obs_view"], s["obs_feature"], s["edges"], s["rel"])
        _cache[name] = (s, r)
    return _cache[name]


def recovery_bound(r):
    """8 n eps lambda_max / (lambda_2 - lambda_1) of the reference's spectrum: Davis-Kahan with the factor's rounding."""
    w = r["eigenvalues"]
    return 8.0 * len(w) * np.finfo(float).eps * w[-1] / (w[1] - w[0])
