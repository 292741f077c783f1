"""Synthetic scenes for LeastUnsquaredDeviationPositionEstimator, modelled on
least_unsquared_deviation_position_estimator_test.cc:50-216: orientations 0.2 * uniform [-1, 1]^3, positions
10 * uniform [-1, 1]^3, chain pairs (i - 1, i) first, then random pairs (first id smaller, no repeats), and per pair
position_2 = N R_1 (c_2 - c_1) / |c_2 - c_1| with N a rotation by noise_deg * uniform [-1, 1] degrees about a random
axis.  The estimator is given the true orientations, as in the reference test.  Optional outlier pairs (never on the
chain) get a random unit direction instead."""
import numpy as np

from tests.rotation_averaging_ref import aa_to_R


def make_scene(num_views, num_pairs, noise_deg=0.0, outlier_fraction=0.0, seed=0):
    rng = np.random.default_rng(seed)
    n = int(num_views)
    orient = 0.2 * rng.uniform(-1.0, 1.0, size=(n, 3))
    pos = 10.0 * rng.uniform(-1.0, 1.0, size=(n, 3))
    pairs = [(i - 1, i) for i in range(1, n)]
    seen = set(pairs)
    target = min(int(num_pairs), n * (n - 1) // 2)
    while len(pairs) < target:
        a, b = (int(v) for v in rng.integers(0, n, size=2))
        a, b = min(a, b), max(a, b)
        if a == b or (a, b) in seen:
            continue
        seen.add((a, b))
        pairs.append((a, b))
    edges = np.array(pairs, dtype=np.int32).reshape(-1, 2)
    E = edges.shape[0]
    R = aa_to_R(orient)
    dirs = pos[edges[:, 1]] - pos[edges[:, 0]]
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    t = np.einsum("eij,ej->ei", R[edges[:, 0]], dirs)
    axis = rng.uniform(-1.0, 1.0, size=(E, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    ang = np.radians(noise_deg * rng.uniform(-1.0, 1.0, size=E))
    t = np.einsum("eij,ej->ei", aa_to_R(ang[:, None] * axis), t)
    outliers = np.zeros(E, dtype=bool)
    if outlier_fraction > 0.0 and E > n - 1:
        cand = np.arange(n - 1, E)
        pick = rng.choice(cand, size=min(len(cand), int(round(outlier_fraction * E))), replace=False)
        outliers[pick] = True
        v = rng.standard_normal((len(pick), 3))
        t[pick] = v / np.linalg.norm(v, axis=1, keepdims=True)
    return dict(n=n, edges=edges, rel=t, orientations=orient, gt=pos, outliers=outliers)


def with_duplicates(scene, num_dup, num_rev, seed=0):
    """The same scene with `num_dup` pairs repeated and `num_rev` pairs added reversed ((j, i) with position_2 =
    -R_j R_i' t_ij), after the original pairs."""
    rng = np.random.default_rng(seed)
    edges, t = scene["edges"], scene["rel"]
    E = edges.shape[0]
    dsel = rng.choice(E, size=num_dup, replace=False)
    rsel = rng.choice(E, size=num_rev, replace=False)
    R = aa_to_R(scene["orientations"])
    er = edges[rsel]
    trev = -np.einsum("eij,ekj,ek->ei", R[er[:, 1]], R[er[:, 0]], t[rsel])
    out = dict(scene)
    out.update(edges=np.ascontiguousarray(np.concatenate([edges, edges[dsel], er[:, ::-1]]).astype(np.int32)),
               rel=np.concatenate([t, t[dsel], trev]))
    return out


def umeyama(src, dst):
    """Similarity (s, R, t) minimising |dst - (s R src + t)| (AlignPointCloudsUmeyama)."""
    src, dst = np.asarray(src, dtype=np.float64), np.asarray(dst, dtype=np.float64)
    ms, md = src.mean(0), dst.mean(0)
    a, b = src - ms, dst - md
    C = b.T @ a / len(src)
    U, sv, Vt = np.linalg.svd(C)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
    R = U @ D @ Vt
    var = (a * a).sum() / len(src)
    s = np.trace(np.diag(sv) @ D) / var
    return s, R, md - s * R @ ms


def aligned_errors(est, gt):
    """AlignPositions then |c_gt - c_est| per view."""
    s, R, t = umeyama(est, gt)
    return np.linalg.norm(gt - (s * np.asarray(est) @ R.T + t), axis=1)


def extent(pos):
    """The scene's extent: the largest distance of a position from their mean."""
    p = np.asarray(pos, dtype=np.float64)
    return float(np.linalg.norm(p - p.mean(0), axis=1).max())
