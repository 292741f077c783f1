"""Scenes for the reconstruction-alignment tests (tests/test_alignment.py, tests/test_alignment_gpu.py): planted similarities
with rotations over all of SO(3), point-cloud batches that straddle the device's paths, camera-correspondence problems for the
CameraAlignmentEstimator, and pairs of array-backed reconstructions that share views by name."""
import numpy as np

from tests import alignment_ref as ar
from tests.wide_rotation_scenes import full_sphere_orientations

PI = float(np.pi)
# the sizes of the batched Umeyama call: one point; three collinear; four coplanar; four in general position; the edges of a
# wavefront (64 lanes), of the one-wavefront path and of a workgroup (256), and the stride loop of the workgroup path
UMEYAMA_SIZES = [1, 3, 4, 4, 63, 64, 65, 257, 4097]
UMEYAMA_KINDS = ["point", "collinear", "coplanar", "general", "cloud", "cloud", "cloud", "cloud", "cloud"]


def rotation(aa):
    return np.asarray(ar.rotation_ld(aa)[0], dtype=np.float64)


def near_pi(rng, gap=1e-3):
    """an angle-axis vector whose angle is within `gap` of pi"""
    ax = rng.standard_normal(3); ax /= np.linalg.norm(ax)
    return ax * (PI - gap * rng.uniform(0.1, 1.0))


def umeyama_batch(seed=20):
    """dict(left, right, weights (lists), planted (R, t, s, reflection) per problem).  Left coordinates lie in [-5, 5]; scales
    run over 1e-2 .. 1e2; the rotations are full_sphere_orientations' (planted half turns included) with two within 1e-3 of
    pi; problem 5 is a planted reflection; problems 4, 6 and 8 carry weights with zeros (the others all ones)."""
    rng = np.random.default_rng(seed)
    aas = full_sphere_orientations(len(UMEYAMA_SIZES), seed)
    aas[6] = near_pi(rng); aas[8] = near_pi(rng)
    scales = [1.0, 1.0, 1.0, 1e-2, 1e2, 3.0, 0.25, 1e-2, 1e2]
    lefts, rights, weights, planted = [], [], [], []
    for p, (n, kind) in enumerate(zip(UMEYAMA_SIZES, UMEYAMA_KINDS)):
        if kind == "point":
            left = rng.uniform(-5, 5, (1, 3))
        elif kind == "collinear":
            a, d = rng.uniform(-5, 5, 3), rng.uniform(-1, 1, 3)
            left = a + np.array([[0.0], [1.0], [-1.7]]) * d
        elif kind == "coplanar":
            a, u, v = rng.uniform(-2, 2, 3), rng.uniform(-1, 1, 3), rng.uniform(-1, 1, 3)
            left = a + np.array([[0.0, 0.0], [2.0, 0.0], [0.0, 2.0], [1.5, -1.0]]) @ np.stack([u, v])
        elif kind == "general":
            left = np.array([[0.0, 0.0, 0.0], [4.0, 0.0, 0.0], [0.0, 4.0, 0.0], [0.0, 0.0, 4.0]]) + rng.uniform(-0.5, 0.5, (4, 3))
        else:
            left = rng.uniform(-5, 5, (n, 3))
        R = rotation(aas[p])
        reflect = p == 5
        M = R @ np.diag([1.0, 1.0, -1.0]) if reflect else R
        t = rng.uniform(-5, 5, 3)
        right = scales[p] * left @ M.T + t
        w = np.ones(n)
        if p in (4, 6, 8):
            w = rng.uniform(0.2, 2.0, n)
            w[rng.choice(n, n // 4, replace=False)] = 0.0
        lefts.append(left); rights.append(right); weights.append(w); planted.append((R, t, scales[p], reflect))
    return dict(left=lefts, right=rights, weights=weights, planted=planted)


def planted_similarity(rng, angle=None):
    ax = rng.standard_normal(3); ax /= np.linalg.norm(ax)
    R = rotation(ax * (rng.uniform(0.0, PI) if angle is None else angle))
    return R, rng.uniform(-3, 3, 3), float(10 ** rng.uniform(-0.5, 0.5))


def camera_problem(rng, n=48, num_outliers=12, noise=1e-3):
    """rows [n][6] = camera1 | camera2 with camera1 = s R camera2 + t + uniform noise in [-noise, noise]^3, but for
    num_outliers rows whose camera1 is displaced by 1 .. 3 units per axis.  Returns (rows, planted inlier mask, (R, t, s))."""
    R, t, s = planted_similarity(rng)
    c2 = rng.uniform(-5, 5, (n, 3))
    c1 = s * c2 @ R.T + t + rng.uniform(-noise, noise, (n, 3))
    out = np.zeros(n, dtype=bool)
    out[rng.choice(n, num_outliers, replace=False)] = True
    c1[out] += rng.uniform(1.0, 3.0, (num_outliers, 3)) * rng.choice([-1.0, 1.0], (num_outliers, 3))
    return np.hstack([c1, c2]), ~out, (R, t, s)


def make_sample_coplanar(rows, inliers, sim, idx, rng, noise=1e-3):
    """camera2 of the four rows `idx` moved into one plane; their camera1 follows the planted similarity (outliers keep their
    displacement class: they stay outliers)"""
    R, t, s = sim
    rows = rows.copy()
    a, u, v = rng.uniform(-2, 2, 3), rng.uniform(-1, 1, 3), rng.uniform(-1, 1, 3)
    c2 = a + np.array([[0.0, 0.0], [3.0, 0.5], [-1.0, 2.5], [2.0, -2.0]]) @ np.stack([u, v])
    for k, i in enumerate(idx):
        rows[i, 3:6] = c2[k]
        rows[i, 0:3] = s * R @ c2[k] + t + rng.uniform(-noise, noise, 3)
        if not inliers[i]:
            rows[i, 0:3] += rng.uniform(1.0, 3.0, 3) * rng.choice([-1.0, 1.0], 3)
    return rows


def reconstruction_pair(displaced=8, seed=3, noise=1e-3):
    """Two sfm.Reconstruction of 40 views and 300 points: rec2 = the planted similarity's inverse image of rec1 (so that
    aligning rec2 to rec1 recovers (R, t, s)), 30 views common by name, `displaced` of those moved by 1 .. 3 units per axis in
    rec2's frame; uniform noise in [-noise, noise]^3 on rec1's common positions.  Returns (rec1, rec2, (R, t, s), common names,
    names of the displaced views)."""
    from pytheiasfm_amd import sfm
    rng = np.random.default_rng(seed)
    R, t, s = planted_similarity(rng)
    nv, nt = 40, 300
    pos2 = rng.uniform(-5, 5, (nv, 3))
    aa2 = full_sphere_orientations(nv, seed + 1)
    pts2 = np.hstack([rng.uniform(-5, 5, (nt, 3)), np.ones((nt, 1))])

    def rec(pos, aa, pts, names):
        r = sfm.Reconstruction()
        r.cam_ext = np.ascontiguousarray(np.hstack([pos, aa]))
        r.view_estimated = np.ones(len(pos), dtype=bool)
        r.points = np.ascontiguousarray(pts)
        r.track_estimated = np.ones(len(pts), dtype=bool)
        r.view_names = list(names)
        return r
    names2 = [f"view_{i:03d}.jpg" for i in range(nv)]
    # rec1: views 10 .. 39 of rec2 (30 in common) in another order, plus ten of its own
    order = rng.permutation(np.arange(10, 40))
    pos1 = s * pos2[order] @ R.T + t + rng.uniform(-noise, noise, (30, 3))
    aa1 = np.zeros((30, 3))
    own = rng.uniform(-5, 5, (10, 3))
    names1 = [names2[i] for i in order] + [f"other_{i:03d}.jpg" for i in range(10)]
    rec1 = rec(np.vstack([pos1, own]), np.vstack([aa1, np.zeros((10, 3))]), np.hstack([rng.uniform(-5, 5, (nt, 3)), np.ones((nt, 1))]), names1)
    moved = [names2[i] for i in order[:displaced]]
    for i in order[:displaced]:
        pos2[i] += rng.uniform(1.0, 3.0, 3) * rng.choice([-1.0, 1.0], 3)
    rec2 = rec(pos2, aa2, pts2, names2)
    return rec1, rec2, (R, t, s), [names2[i] for i in order], moved


ALIGN_ROTATION_SIZES = [1, 2, 65, 1000]
# name -> (angle of the planted alignment, noise): at 0 without noise there is nothing to align; 3 rad is where the
# reference's residual (a difference of angle-axis vectors) wraps
ALIGN_ROTATION_CASES = {"zero_exact": (0.0, 0.0), "zero": (0.0, 1e-3), "one_radian": (1.0, 1e-3), "three_radians": (3.0, 1e-3)}


def align_rotations_scene(n, name, seed=0):
    """(gt [n][3], rotation [n][3], planted w): rotation_i R(w) = gt_i up to uniform noise in [-noise, noise]^3 on the
    rotation's angle-axis vector.  gt has angles up to 2 rad, so that with the alignments up to 1 rad no rotation of the
    problem comes near a half turn."""
    from tests.rotation_averaging_ref import aa_to_R, R_to_aa
    angle, noise = ALIGN_ROTATION_CASES[name]
    rng = np.random.default_rng(1000 * seed + 10 * n + list(ALIGN_ROTATION_CASES).index(name))
    ax = rng.standard_normal((n, 3)); ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    gt = ax * rng.uniform(0.0, 2.0, (n, 1))
    wa = rng.standard_normal(3); wa *= angle / np.linalg.norm(wa)
    rot = gt.copy() if angle == 0.0 else R_to_aa(aa_to_R(gt) @ rotation(wa).T)
    rot = rot + rng.uniform(-noise, noise, (n, 3))
    return gt, rot, wa
