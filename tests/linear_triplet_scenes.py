"""Synthetic scenes of the linear triplet position tests, in the set-up of the reference's own test unless a case needs
otherwise: camera positions 10 U(-1, 1)^3, orientations (angle-axis) 0.2 U(-1, 1)^3, points U(-1, 1)^3 + (0, 0, 20); a
view pair (i < j) carries rotation_2 = log(R_j R_i') and position_2 = R_i (c_j - c_i) / |.|; a track is seen by a stated
set of views and its feature is hnormalized(R (X - c)).  The noisy variants turn every position_2 by 1 degree about a
random axis.  Every scene exists because a kernel of csrc/linear_positions.hip can go wrong there:

    v4_full             4 views, 6 pairs, 50 tracks seen by all: the reference's own test
    v12_sparse          a strip of triangles with 1, 2, 63, 64, 65 and 130 common tracks (wave boundaries, even and odd
                        k), one triangle without a common track (state 1) that cuts the triangle behind it off (state
                        2), a separate triangle, two edges in no triangle, tracks seen by three and by four views
    v10_gate            views 0 and 1 are 0.3 apart and the points 4.5 .. 16 deep: the 2 degree test rejects some tracks
                        of that pair and accepts others (the cameras lie near a plane so that every point is in front)
    v14_two_components  the complete graphs on views 0 .. 7 and 8 .. 13, the triangle (7, 8, 9) that hangs the second
                        cluster on view 7, and the bridge (0, 13) in no triangle: the smaller cluster is state 2
    v70_hub             view 0 adjacent to all 69 others and the chain i - (i + 1): 68 triangles
    v9_collinear        view 1 is the midpoint of views 0 and 2: the antiparallel branch of FromTwoVectors
    v12_flip            v12_strip with every position_2 negated: the lines of the midpoint solve do not see the sign, so
                        the system is the same to the bit and only the vote turns
"""
import numpy as np

from tests import linear_triplet_ref as ref


def log_rotation(R):
    """Angle-axis of a rotation matrix (angles well below pi here)."""
    c = min(1.0, max(-1.0, (np.trace(R) - 1.0) / 2.0))
    th = np.arccos(c)
    v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    if th < 1e-12:
        return 0.5 * v
    return th / (2.0 * np.sin(th)) * v


def assemble(pos, aa, pairs, tracks, pts, rng, noise_deg=0.0, negate=False):
    """pairs: (i < j) list; tracks: list of view lists, track t observing pts[t]."""
    R = np.array([ref.rotation_matrix(w) for w in aa])
    edges = np.array(sorted(set((min(i, j), max(i, j)) for i, j in pairs)), dtype=np.int32)
    perm = rng.permutation(len(edges))          # the caller's edge order is arbitrary
    edges = edges[perm]
    rot = np.array([log_rotation(R[j] @ R[i].T) for i, j in edges])
    rel = np.array([R[i] @ (pos[j] - pos[i]) / np.linalg.norm(pos[j] - pos[i]) for i, j in edges])
    if noise_deg > 0.0:
        for k in range(len(rel)):
            axis = rng.standard_normal(3)
            rel[k] = ref.rotation_matrix(np.deg2rad(noise_deg) * axis / np.linalg.norm(axis)) @ rel[k]
    if negate:
        rel = -rel
    obs_view, obs_feat, offsets = [], [], [0]
    for t, views in enumerate(tracks):
        for v in views:
            p = R[v] @ (pts[t] - pos[v])
            obs_view.append(v)
            obs_feat.append(p[:2] / p[2])
        offsets.append(len(obs_view))
    return dict(orientations=aa, positions=pos, edges=edges, rot=rot, rel=rel,
                track_offsets=np.array(offsets, dtype=np.int32), obs_view=np.array(obs_view, dtype=np.int32),
                obs_feature=np.array(obs_feat).reshape(-1, 2), num_views=len(pos), noise=noise_deg)


def _cameras(rng, n):
    return 10.0 * rng.uniform(-1, 1, (n, 3)), 0.2 * rng.uniform(-1, 1, (n, 3))


def _points(rng, k):
    return rng.uniform(-1, 1, (k, 3)) + np.array([0.0, 0.0, 20.0])


def _complete(views):
    views = list(views)
    return [(a, b) for i, a in enumerate(views) for b in views[i + 1:]]


def _shuffled(rng, views):
    return [int(v) for v in rng.permutation(list(views))]


def v4_full(seed=21, noise_deg=0.0):
    rng = np.random.default_rng(seed)
    pos, aa = _cameras(rng, 4)
    tracks = [_shuffled(rng, range(4)) for _ in range(50)]
    return assemble(pos, aa, _complete(range(4)), tracks, _points(rng, 50), rng, noise_deg)


# v12_sparse: triangle -> tracks seen by exactly its three views; 5 more tracks are seen by views 2, 3, 4, 5
SPARSE_EXCLUSIVE = {(0, 1, 2): 1, (1, 2, 3): 2, (2, 3, 4): 58, (3, 4, 5): 59, (4, 5, 6): 65, (5, 6, 7): 130, (6, 7, 8): 0,
                    (7, 8, 9): 10, (9, 10, 11): 20}
SPARSE_COMMON = {(0, 1, 2): 1, (1, 2, 3): 2, (2, 3, 4): 63, (3, 4, 5): 64, (4, 5, 6): 65, (5, 6, 7): 130, (6, 7, 8): 0,
                 (7, 8, 9): 10, (9, 10, 11): 20}
SPARSE_STATE = {(6, 7, 8): 1, (7, 8, 9): 2, (9, 10, 11): 2}


def v12_sparse(seed=22, noise_deg=0.0):
    rng = np.random.default_rng(seed)
    pos, aa = _cameras(rng, 12)
    pairs = [(0, 11), (3, 9)]                     # in no triangle
    tracks = []
    for tri, k in SPARSE_EXCLUSIVE.items():
        pairs += _complete(tri)
        tracks += [_shuffled(rng, tri) for _ in range(k)]
    tracks += [_shuffled(rng, (2, 3, 4, 5)) for _ in range(5)]
    tracks += [[6, 8], [7]]                       # shorter than a triangle
    order = rng.permutation(len(tracks))
    tracks = [tracks[k] for k in order]
    return assemble(pos, aa, pairs, tracks, _points(rng, len(tracks)), rng, noise_deg)


def v10_gate(seed=23):
    rng = np.random.default_rng(seed)
    pos, aa = _cameras(rng, 10)
    pos[:, 2] = rng.uniform(-1, 1, 10)
    pos[1] = pos[0] + np.array([0.3, 0.0, 0.0])
    pts = np.column_stack([3.0 * rng.uniform(-1, 1, (60, 2)), rng.uniform(4.5, 16.0, 60)])
    tracks = [_shuffled(rng, range(10)) for _ in range(60)]
    return assemble(pos, aa, _complete(range(10)), tracks, pts, rng)


def v14_two_components(seed=24):
    rng = np.random.default_rng(seed)
    pos, aa = _cameras(rng, 14)
    pairs = _complete(range(8)) + _complete(range(8, 14)) + [(7, 8), (7, 9), (0, 13)]
    tracks = [_shuffled(rng, range(8)) for _ in range(40)] + [_shuffled(rng, range(7, 14)) for _ in range(40)]
    return assemble(pos, aa, pairs, tracks, _points(rng, 80), rng)


def v70_hub(seed=65):
    rng = np.random.default_rng(seed)
    pos, aa = _cameras(rng, 70)
    pairs = [(0, i) for i in range(1, 70)] + [(i, i + 1) for i in range(1, 69)]
    tracks = []
    for i in range(1, 69):
        tracks += [_shuffled(rng, (0, i, i + 1)) for _ in range(6)]
    order = rng.permutation(len(tracks))
    tracks = [tracks[k] for k in order]
    return assemble(pos, aa, pairs, tracks, _points(rng, len(tracks)), rng)


def v9_collinear(seed=26):
    rng = np.random.default_rng(seed)
    pos, aa = _cameras(rng, 9)
    pos[1] = 0.5 * (pos[0] + pos[2])
    tracks = [_shuffled(rng, range(9)) for _ in range(40)]
    return assemble(pos, aa, _complete(range(9)), tracks, _points(rng, 40), rng)


def v12_strip(seed=27, negate=False):
    rng = np.random.default_rng(seed)
    pos, aa = _cameras(rng, 12)
    pos[0] = (-9.0, -9.0, -9.0)                   # held: the other positions relative to it sum to a positive number
    pairs = [(i, i + 1) for i in range(11)] + [(i, i + 2) for i in range(10)] + [(0, 5), (3, 8)]
    tracks = [_shuffled(rng, range(12)) for _ in range(30)]
    return assemble(pos, aa, pairs, tracks, _points(rng, 30), rng, negate=negate)


SCENES = {
    "v4_full": lambda: v4_full(),
    "v12_sparse": lambda: v12_sparse(),
    "v10_gate": lambda: v10_gate(),
    "v14_two_components": lambda: v14_two_components(),
    "v70_hub": lambda: v70_hub(),
    "v9_collinear": lambda: v9_collinear(),
    "v12_strip": lambda: v12_strip(),
    "v12_flip": lambda: v12_strip(negate=True),
    "v4_full_noisy": lambda: v4_full(noise_deg=1.0),
    "v12_sparse_noisy": lambda: v12_sparse(noise_deg=1.0),
}
NOISE_FREE = ("v4_full", "v12_sparse", "v10_gate", "v14_two_components", "v70_hub", "v9_collinear", "v12_strip")
NOISY = ("v4_full_noisy", "v12_sparse_noisy")

_cache = {}


def scene(name):
    """The scene and its restated solution, computed once and shared: (scene dict, linear_triplet_ref.estimate dict).
    Neither is to be modified."""
    if name not in _cache:
        s = SCENES[name]()
        r = ref.estimate(s["orientations"], s["edges"], s["rot"], s["rel"], s["track_offsets"], s["obs_view"],
                         s["obs_feature"])
        _cache[name] = (s, r)
    return _cache[name]


def fit(scene_, positions, estimated, index):
    """positions = s (c - c_held): the least-squares s and the largest view error relative to |s (c - c_held)|_2."""
    held = int(np.nonzero(index == -1)[0][0])
    d = (scene_["positions"] - scene_["positions"][held])[estimated]
    p = positions[estimated]
    s = float((p * d).sum() / (d * d).sum())
    return s, float(np.linalg.norm(p - s * d, axis=1).max() / np.linalg.norm(s * d))


def recovery_bound(r):
    """Davis-Kahan: |dH|_2 / (lambda_2 - lambda_1).  dH has the factorisation's 8 n eps lambda_max, as in
    ligt_scenes.recovery_bound, and the entrywise h_bound of the assembly, which carries the medians' conditioning
    (2 / (1 - (d0 . d1)^2) per midpoint); |h_bound|_2 <= its Frobenius norm."""
    w = r["eigenvalues"]
    dH = 8.0 * len(w) * np.finfo(float).eps * w[-1] + np.linalg.norm(r["h_bound"])
    return dH / (w[1] - w[0])
