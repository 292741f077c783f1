"""Synthetic view graphs for RobustRotationEstimator, modelled on robust_rotation_estimator_test.cc:63-165:
random ground-truth orientations (0.2 * uniform [-1, 1]^3), chain edges (i - 1, i) first, then random pairs (first id
smaller, no repeats), relative rotations R_ij = N R_j R_i^T with N a rotation by `noise_deg` about a random axis,
optional outlier edges (a random rotation in place of R_ij, never on the chain), and initial orientations chained
along (i - 1, i) from view 0 at the identity."""
import numpy as np

from tests.rotation_averaging_ref import aa_to_R, R_to_aa


def make_scene(num_views, num_pairs, noise_deg=0.0, outlier_fraction=0.0, seed=0):
    rng = np.random.default_rng(seed)
    n = int(num_views)
    gt = 0.2 * rng.uniform(-1.0, 1.0, size=(n, 3))
    Rgt = aa_to_R(gt)
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
    axis = rng.uniform(-1.0, 1.0, size=(E, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    N = aa_to_R(np.radians(noise_deg) * axis)
    rel = R_to_aa(N @ Rgt[edges[:, 1]] @ np.transpose(Rgt[edges[:, 0]], (0, 2, 1)))
    outliers = np.zeros(E, dtype=bool)
    if outlier_fraction > 0.0 and E > n - 1:
        cand = np.arange(n - 1, E)
        pick = rng.choice(cand, size=min(len(cand), int(round(outlier_fraction * E))), replace=False)
        outliers[pick] = True
        for k in pick:
            axis = rng.uniform(-1.0, 1.0, size=3)
            rel[k] = rng.uniform(0.3, 3.0) * axis / np.linalg.norm(axis)
    init = chain_init(n, edges, rel)
    return dict(n=n, edges=edges, rel=rel, gt=gt, init=init, outliers=outliers)


def chain_init(n, edges, rel):
    """InitializeRotationsFromSpanningTree: view 0 at the origin, view i = R_(i-1,i) applied to view i - 1 (the chain edges
    are the first n - 1 edges)."""
    init = np.zeros((n, 3))
    for i in range(1, n):
        a, b = edges[i - 1]
        assert (a, b) == (i - 1, i)
        R = aa_to_R(rel[i - 1][None])[0] @ aa_to_R(init[i - 1][None])[0]
        init[i] = R_to_aa(R[None])[0]
    return init


def with_duplicates(scene, num_dup, num_rev, seed=0):
    """The same scene with `num_dup` edges repeated and `num_rev` edges added reversed ((j, i) with R_ij^T), after the
    original edges so that the chain initialisation is unchanged."""
    rng = np.random.default_rng(seed)
    E = scene["edges"].shape[0]
    d = rng.choice(E, size=num_dup, replace=False)
    r = rng.choice(E, size=num_rev, replace=False)
    edges = np.concatenate([scene["edges"], scene["edges"][d], scene["edges"][r][:, ::-1]]).astype(np.int32)
    rel = np.concatenate([scene["rel"], scene["rel"][d], -scene["rel"][r]])
    out = dict(scene)
    out.update(edges=np.ascontiguousarray(edges), rel=rel)
    return out


def aligned_errors_deg(est, gt):
    """AlignOrientations then the angle of R_est R_gt^T per view, degrees.  The alignment is the rotation that maps the
    estimate's frame to the ground truth's, averaged over the views (chordal mean of R_gt_i^T R_est_i, projected on SO(3))."""
    Re, Rg = aa_to_R(est), aa_to_R(gt)
    M = np.einsum("nji,njk->ik", Rg, Re)   # sum_i Rg_i^T Re_i
    U, _, Vt = np.linalg.svd(M)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
    C = U @ D @ Vt                          # Re_i ~ Rg_i C  =>  Re_i C^T ~ Rg_i
    return np.degrees(_angle_of(np.einsum("nij,kj->nik", Re, C) @ np.transpose(Rg, (0, 2, 1))))


def angle_between(a, b):
    """Per-row angle (rad) of R(a) R(b)^T."""
    return _angle_of(np.einsum("nij,nkj->nik", aa_to_R(a), aa_to_R(b)))


def _angle_of(d):
    """Rotation angle of rows of d [n][3][3], by atan2 of the axis part and the trace (acos loses precision near 0)."""
    c = np.clip((np.trace(d, axis1=1, axis2=2) - 1.0) / 2.0, -1.0, 1.0)
    s = 0.5 * np.linalg.norm(np.stack([d[:, 2, 1] - d[:, 1, 2], d[:, 0, 2] - d[:, 2, 0], d[:, 1, 0] - d[:, 0, 1]], 1), axis=1)
    return np.arctan2(s, c)
