"""Scenes whose orientations cover all of SO(3), for the global-pose stages.  The scenes copied from the reference's unit
tests (rotation_scenes, position_scenes, ligt_scenes, linear_triplet_scenes) turn no view by more than 20 degrees; a
reconstruction of an object the cameras walk around has world-to-camera rotations of every angle up to pi and relative
rotations just as large, and that is where the rotation maps of csrc/ have most of their branches.

    full_sphere_orientations   unit axis from a normal draw, angle U(0, pi); from 8 rows on, rows 1 .. 7 are PLANTED
    wide_rotation_scene        the contract of rotation_scenes.make_scene on those orientations, with planted outliers
    wide_position_scene        the contract of position_scenes.make_scene on those orientations
    orbit_cameras              cameras on a shell about the origin, each looking at it with a random roll
    orbit_ligt_scene           the contract of ligt_scenes.make_scene on orbit cameras
    orbit_triplet_scene        the contract of linear_triplet_scenes.assemble on orbit cameras
    orientation_filter_scene   pairs whose rotation_2 is off the true relative rotation by angles on both sides of a threshold

Every relative rotation goes through rotation_averaging_ref.R_to_aa, the logarithm that is valid up to pi."""
import numpy as np

from tests import ligt_positions_ref
from tests import linear_triplet_scenes as lts
from tests.rotation_averaging_ref import aa_to_R, R_to_aa
from tests.rotation_scenes import chain_init

PI = float(np.pi)
# rows 1 .. 7 of full_sphere_orientations(n >= 8): half turns about the coordinate axes and the diagonal (the diagonal:
# three equal diagonal entries of -1/3), a hair under a half turn, a non-zero vector inside ceres' small-angle branch, zero
PLANTED = np.array([[PI, 0.0, 0.0], [0.0, PI, 0.0], [0.0, 0.0, PI], [PI / np.sqrt(3.0)] * 3, [PI - 1e-9, 0.0, 0.0],
                    [1e-9, 0.0, 0.0], [0.0, 0.0, 0.0]])


def full_sphere_orientations(n, seed):
    rng = np.random.default_rng(seed)
    axis = rng.standard_normal((n, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    aa = rng.uniform(0.0, PI, size=n)[:, None] * axis
    if n >= 8:
        aa[1:8] = PLANTED
    return aa


def _pairs(rng, n, num_pairs):
    """Chain pairs (i - 1, i) first, then random pairs (first id smaller, no repeats)."""
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
    return np.array(pairs, dtype=np.int32).reshape(-1, 2)


def _unit(rng, k):
    v = rng.standard_normal((k, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def wide_rotation_scene(num_views, num_pairs, noise_deg=0.0, outlier_fraction=0.0, seed=0):
    """dict(n, edges, rel, gt, init, outliers) as rotation_scenes.make_scene.  Outlier q (never on the chain) gets
    rel = A_q N R_j R_i^T with A_q a rotation of U(2.2, 3.1) rad about coordinate axis q % 3: at the ground truth its
    residual is A_q^T, so each of the three largest-diagonal branches of the logarithm gets a third of the outliers."""
    rng = np.random.default_rng((seed, 1))   # the orientations take the stream of `seed` itself
    n = int(num_views)
    gt = full_sphere_orientations(n, seed)
    Rgt = aa_to_R(gt)
    edges = _pairs(rng, n, num_pairs)
    E = edges.shape[0]
    N = aa_to_R(np.radians(noise_deg) * _unit(rng, E))
    Rrel = N @ Rgt[edges[:, 1]] @ np.transpose(Rgt[edges[:, 0]], (0, 2, 1))
    outliers = np.zeros(E, dtype=bool)
    if outlier_fraction > 0.0 and E > n - 1:
        cand = np.arange(n - 1, E)
        pick = np.sort(rng.choice(cand, size=min(len(cand), int(round(outlier_fraction * E))), replace=False))
        outliers[pick] = True
        turn = np.zeros((len(pick), 3))
        turn[np.arange(len(pick)), np.arange(len(pick)) % 3] = rng.uniform(2.2, 3.1, size=len(pick))
        Rrel[pick] = aa_to_R(turn) @ Rrel[pick]
    rel = R_to_aa(Rrel)
    return dict(n=n, edges=edges, rel=rel, gt=gt, init=chain_init(n, edges, rel), outliers=outliers)


def noisy_start(scene, noise_deg, held, seed=0):
    """The ground truth turned by `noise_deg` about a random axis per view, the held views exactly at the ground truth."""
    rng = np.random.default_rng(seed)
    N = aa_to_R(np.radians(noise_deg) * _unit(rng, scene["n"]))
    x0 = R_to_aa(N @ aa_to_R(scene["gt"]))
    x0[held] = scene["gt"][held]
    return x0


def log_branch(E):
    """The branch ceres::RotationMatrixToQuaternion takes on E [3][3] (0: trace >= 0; 1 + i: the largest diagonal entry is
    i) and how far the deciding comparisons are from a tie: |trace|, and on a diagonal branch the smallest difference
    between the chosen diagonal entry and the other two."""
    d = np.diag(E)
    trace = float(d.sum())
    if trace >= 0.0:
        return 0, abs(trace)
    i = 0
    if d[1] > d[0]:
        i = 1
    if d[2] > d[i]:
        i = 2
    return 1 + i, min(abs(trace), min(float(d[i] - d[k]) for k in range(3) if k != i))


def residual_branches(x, edges, rel):
    """log_branch of R(x_j) R(x_i)^T R(rel)^T per edge: (branch [E], margin [E])."""
    R, Rr = aa_to_R(x), aa_to_R(rel)
    Em = R[edges[:, 1]] @ np.transpose(R[edges[:, 0]], (0, 2, 1)) @ np.transpose(Rr, (0, 2, 1))
    out = [log_branch(M) for M in Em]
    return np.array([b for b, _ in out]), np.array([m for _, m in out])


def wide_position_scene(num_views, num_pairs, noise_deg=0.0, outlier_fraction=0.0, seed=0):
    """dict(n, edges, rel, orientations, gt, outliers) as position_scenes.make_scene: positions 10 U(-1, 1)^3,
    position_2 = N R_1 (c_2 - c_1) / |c_2 - c_1|, outlier pairs (never on the chain) a random unit direction."""
    rng = np.random.default_rng((seed, 1))   # the orientations take the stream of `seed` itself
    n = int(num_views)
    orient = full_sphere_orientations(n, seed)
    pos = 10.0 * rng.uniform(-1.0, 1.0, size=(n, 3))
    edges = _pairs(rng, n, num_pairs)
    E = edges.shape[0]
    dirs = pos[edges[:, 1]] - pos[edges[:, 0]]
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    t = np.einsum("eij,ej->ei", aa_to_R(orient)[edges[:, 0]], dirs)
    ang = np.radians(noise_deg * rng.uniform(-1.0, 1.0, size=E))
    t = np.einsum("eij,ej->ei", aa_to_R(ang[:, None] * _unit(rng, E)), t)
    outliers = np.zeros(E, dtype=bool)
    if outlier_fraction > 0.0 and E > n - 1:
        pick = rng.choice(np.arange(n - 1, E), size=min(E - n + 1, int(round(outlier_fraction * E))), replace=False)
        outliers[pick] = True
        t[pick] = _unit(rng, len(pick))
    return dict(n=n, edges=edges, rel=t, orientations=orient, gt=pos, outliers=outliers)


def as_filter_scene(s):
    """A wide_position_scene under the names of filter_scenes.position_scene."""
    return dict(n=s["n"], pairs=s["edges"], orientations=s["orientations"], positions=s["gt"], position_2=s["rel"],
                invalid=s["outliers"], num_valid=int((~s["outliers"]).sum()))


def orientation_filter_scene(num_views, num_pairs, max_degrees, seed=0):
    """dict(n, edges, orientations, rel, turned_deg): rotation_2 = T R_2 R_1^T with T a rotation about a random axis by
    max_degrees * U(0.25, 1.75) -- both sides of the threshold -- and, for every fourth pair, about a coordinate axis by
    U(2.2, 3.1) rad, which sends the loop's logarithm through its three largest-diagonal branches."""
    rng = np.random.default_rng((seed, 1))   # the orientations take the stream of `seed` itself
    n = int(num_views)
    orient = full_sphere_orientations(n, seed)
    R = aa_to_R(orient)
    edges = _pairs(rng, n, num_pairs)
    E = edges.shape[0]
    turn = np.radians(max_degrees * rng.uniform(0.25, 1.75, size=E))[:, None] * _unit(rng, E)
    far = np.arange(0, E, 4)
    turn[far] = 0.0
    turn[far, np.arange(len(far)) % 3] = rng.uniform(2.2, 3.1, size=len(far))
    rel = R_to_aa(aa_to_R(turn) @ R[edges[:, 1]] @ np.transpose(R[edges[:, 0]], (0, 2, 1)))
    return dict(n=n, edges=edges, orientations=orient, rel=rel, turned_deg=np.degrees(np.linalg.norm(turn, axis=1)))


def orbit_cameras(n, seed, radius=20.0):
    """(positions [n][3], orientations [n][3], rng): positions on a shell of radius * U(0.8, 1.2) about the origin; the
    world-to-camera rotation has the direction to the origin as its third row and a random roll about it."""
    rng = np.random.default_rng(seed)
    pos = _unit(rng, n) * (radius * rng.uniform(0.8, 1.2, size=n))[:, None]
    R = np.empty((n, 3, 3))
    for v in range(n):
        z = -pos[v] / np.linalg.norm(pos[v])
        a = np.eye(3)[int(np.argmin(np.abs(z)))]
        x = np.cross(a, z)
        x /= np.linalg.norm(x)
        y = np.cross(z, x)
        roll = rng.uniform(0.0, 2.0 * PI)
        R[v] = np.stack([np.cos(roll) * x + np.sin(roll) * y, -np.sin(roll) * x + np.cos(roll) * y, z])
    return pos, R_to_aa(R), rng


def orbit_ligt_scene(num_views, num_tracks, obs_per_track, seed):
    """The dict of ligt_scenes.make_scene on orbit cameras: points U(-1, 1)^3 about the origin (in front of every camera),
    a track seen by `obs_per_track` distinct views in a random order, pairs = a ring plus as many random pairs."""
    nv = int(num_views)
    pos, aa, rng = orbit_cameras(nv, seed)
    R = np.array([ligt_positions_ref.rotation_matrix(w) for w in aa])
    pts = rng.uniform(-1, 1, (num_tracks, 3))
    obs_view, obs_feat, offsets = [], [], [0]
    for t in range(num_tracks):
        for v in rng.permutation(nv)[:obs_per_track]:
            p = R[v] @ (pts[t] - pos[v])
            obs_view.append(v)
            obs_feat.append(p[:2] / p[2])
        offsets.append(len(obs_view))
    ring = [(i, (i + 1) % nv) for i in range(nv)]
    rand = [tuple(rng.permutation(nv)[:2]) for _ in range(nv)]
    edges = np.array(ring + rand, dtype=np.int32)
    rel = np.array([R[i] @ (pos[j] - pos[i]) / np.linalg.norm(pos[j] - pos[i]) for i, j in edges])
    return dict(orientations=aa, positions=pos, track_offsets=np.array(offsets, dtype=np.int32),
                obs_view=np.array(obs_view, dtype=np.int32), obs_feature=np.array(obs_feat), edges=edges, rel=rel,
                num_views=nv, noise=0.0)


def orbit_triplet_scene(num_views, seed, graph="complete", num_tracks=40):
    """The dict of linear_triplet_scenes.assemble on orbit cameras, every track seen by all views; graph "complete" or
    "ring2" (ring plus second neighbours).  rotation_2 is taken again with the logarithm that is valid up to pi."""
    n = int(num_views)
    pos, aa, rng = orbit_cameras(n, seed)
    if graph == "complete":
        pairs = [(a, b) for a in range(n) for b in range(a + 1, n)]
    else:
        pairs = [(i, (i + s) % n) for i in range(n) for s in (1, 2)]
    tracks = [[int(v) for v in rng.permutation(n)] for _ in range(num_tracks)]
    s = lts.assemble(pos, aa, pairs, tracks, rng.uniform(-1, 1, (num_tracks, 3)), rng)
    R = aa_to_R(aa)
    e = s["edges"]
    s["rot"] = R_to_aa(R[e[:, 1]] @ np.transpose(R[e[:, 0]], (0, 2, 1)))
    return s


# ---- the cases the CPU tests (fairness of every scene) and the GPU tests (the device against the restatements) share
# name: (views, pairs, noise in degrees, outlier fraction, fixed views, seed)
ROTATION_CASES = {"w12": (12, 40, 1.0, 0.0, 1, 1), "w66_outliers": (66, 500, 2.0, 0.1, 1, 4),
                  "w130_three_fixed": (130, 1200, 2.0, 0.1, 3, 3)}
# name: (views, pairs, noise in degrees, outlier fraction, seed)
NONLINEAR_CASES = {"w22": (22, 80, 2.0, 0.1, 1), "w66": (66, 500, 2.0, 0.1, 6)}
LINEAR_CASES = {"w12_noise_free": (12, 40, 0.0, 0.0, 1), "w12": (12, 40, 1.0, 0.0, 1), "w70": (70, 500, 2.0, 0.0, 4)}
LUD_CASES = {"w23": (23, 90, 2.0, 0.0, 5), "w66": (66, 300, 2.0, 0.1, 8)}
# name: (views, tracks, observations per track, seed)
LIGT_CASES = {"o6": (6, 40, 4, 11), "o20": (20, 200, 5, 12), "o70": (70, 600, 6, 13)}
# name: (views, seed, graph)
TRIPLET_CASES = {"o4": (4, 21, "complete"), "o12": (12, 22, "complete"), "o30": (30, 23, "ring2")}
HELD = np.arange(1, 8)          # the held-views case of the nonlinear estimator: the planted rows of "w22"
FILTER_VIEWS, FILTER_PAIRS, FILTER_DEGREES = 40, 200, 2.0
ORIENTATION_FILTER_SEED, TRANSLATION_FILTER_SEED, TRANSLATION_FILTER_AXES_SEED = 5, 8, 5

_cache = {}


def cached(key, make):
    """make() once per key; what it returns is shared and not to be modified."""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def rotation_case(name):
    n, pairs, noise, out, nfix, seed = ROTATION_CASES[name]
    return cached(("rotation", name), lambda: (wide_rotation_scene(n, pairs, noise, out, seed=seed), np.arange(n) < nfix))


def nonlinear_case(name):
    return cached(("nonlinear", name), lambda: wide_rotation_scene(*NONLINEAR_CASES[name][:4], seed=NONLINEAR_CASES[name][4]))


def linear_case(name):
    return cached(("linear", name), lambda: wide_rotation_scene(*LINEAR_CASES[name][:4], seed=LINEAR_CASES[name][4]))


def lud_case(name):
    return cached(("lud", name), lambda: wide_position_scene(*LUD_CASES[name][:4], seed=LUD_CASES[name][4]))


def ligt_case(name):
    def make():
        s = orbit_ligt_scene(*LIGT_CASES[name])
        return s, ligt_positions_ref.estimate(s["orientations"], s["track_offsets"], s["obs_view"], s["obs_feature"], s["edges"],
                                              s["rel"])
    return cached(("ligt", name), make)


def triplet_case(name):
    def make():
        s = orbit_triplet_scene(*TRIPLET_CASES[name])
        return s, lts.ref.estimate(s["orientations"], s["edges"], s["rot"], s["rel"], s["track_offsets"], s["obs_view"],
                                   s["obs_feature"])
    return cached(("triplet", name), make)


def orientation_filter_case():
    return cached("orientation_filter",
                  lambda: orientation_filter_scene(FILTER_VIEWS, FILTER_PAIRS, FILTER_DEGREES, seed=ORIENTATION_FILTER_SEED))


def translation_filter_case():
    return cached("translation_filter", lambda: as_filter_scene(
        wide_position_scene(FILTER_VIEWS, FILTER_PAIRS, 2.0, 0.1, seed=TRANSLATION_FILTER_SEED)))
