"""numpy restatement of the two view-graph prunings, and the scenes their tests share.

cycle_filter restates FilterViewGraphCyclesByRotation (sfm/filter_view_graph_cycles_by_rotation.cc:54-145) sequentially:
every pair starts invalid (:100-106); the triangles a < b < c are visited one at a time; each chains
loop = R_bc R_ab R_ac' (:70-71) from ceres' AngleAxisToRotationMatrix of the pairs' rotation_2 and takes
RadToDeg(|RotationMatrixToAngleAxis(loop)|) (:72-79); an error below the threshold validates the triangle's three pairs
(:132-134).  Beside the verdicts it keeps what the library reports: the smallest error per pair (a NaN error is no
minimum; +inf where there is none), the triangles per pair and the triangles of the graph.  The stated extension: a pair
listed (b, a) with b > a carries the rotation of that orientation, and its ascending matrix is the transpose.

components restates RemoveDisconnectedViewPairs (sfm/view_graph/remove_disconnected_view_pairs.cc:48-95) as a sequential
union-find with the stated order: the largest component by views stays, among equally large ones the one holding the
smallest view index; a view that no pair names is neither kept nor removed.

Every scene carries the thresholds it is used with, and its builder asserts -- on the restatement alone -- that no finite
per-pair minimum lies within MARGIN degrees of any of them, so that no pair has to be left out of a comparison.
(A threshold of 0, a negative one or NaN is no such threshold: no error is below it, whatever the minima are.)"""
import functools
import math

import numpy as np

from tests.rotation_averaging_ref import aa_to_R, R_to_aa

RAD_TO_DEG = 180.0 / math.pi   # math/util.h:48
MARGIN = 1e-6                  # degrees between a finite per-pair minimum and a threshold the scene is used with


# ---------------------------------------------------------------------------------------------------- restatement
def ascending_matrices(pairs, rotation_2):
    R = aa_to_R(rotation_2)
    for e, (i, j) in enumerate(pairs):
        if i > j:
            R[e] = R[e].T.copy()
    return R


def triangles(num_views, pairs):
    """(a, b, c, e_ab, e_ac, e_bc) for every triangle a < b < c, in ascending (a, b, c)."""
    index = {(min(int(i), int(j)), max(int(i), int(j))): e for e, (i, j) in enumerate(pairs)}
    nb = [set() for _ in range(num_views)]
    for a, b in index:
        nb[a].add(b)
        nb[b].add(a)
    out = []
    for a in range(num_views):
        for b in sorted(v for v in nb[a] if v > a):
            for c in sorted(v for v in nb[a] & nb[b] if v > b):
                out.append((a, b, c, index[(a, b)], index[(a, c)], index[(b, c)]))
    return out


def loop_error_degrees(Rab, Rac, Rbc):
    """ComputeLoopRotationError (:54-80)."""
    loop = Rbc @ Rab @ Rac.T
    with np.errstate(invalid="ignore"):
        return float(np.linalg.norm(R_to_aa(loop[None])[0])) * RAD_TO_DEG


def loop_errors(num_views, pairs, rotation_2):
    """[(e_ab, e_ac, e_bc, error in degrees)], one entry per triangle: what does not depend on the threshold."""
    R = ascending_matrices(pairs, rotation_2)
    return [(ab, ac, bc, loop_error_degrees(R[ab], R[ac], R[bc])) for _, _, _, ab, ac, bc in triangles(num_views, pairs)]


def cycle_filter(num_views, pairs, rotation_2, max_loop_error_degrees, errors=None):
    if errors is None:
        errors = loop_errors(num_views, pairs, rotation_2)
    E = len(pairs)
    invalid = np.ones(E, dtype=bool)
    min_err = np.full(E, np.inf)
    count = np.zeros(E, dtype=np.int32)
    for ab, ac, bc, err in errors:
        for e in (ab, ac, bc):
            count[e] += 1
            if err < min_err[e]:
                min_err[e] = err
        if err < max_loop_error_degrees:
            invalid[[ab, ac, bc]] = False
    return dict(removed=invalid, min_loop_error_degrees=min_err, triangles_per_pair=count, num_triangles=len(errors))


def components(num_views, pairs):
    parent = list(range(num_views))

    def find(v):
        while parent[v] != v:
            v = parent[v]
        return v

    named = np.zeros(num_views, dtype=bool)
    for i, j in pairs:
        named[i] = named[j] = True
        a, b = find(int(i)), find(int(j))
        if a != b:
            parent[max(a, b)] = min(a, b)
    root = np.array([find(v) for v in range(num_views)], dtype=np.int32).reshape(num_views)
    kept, kept_size = -1, 0
    for v in range(num_views):   # ascending, strict: among equally large components the smallest view index wins
        size = int((named & (root == v)).sum())
        if size > kept_size:
            kept, kept_size = v, size
    removed_views = named & (root != kept)
    removed_pairs = np.array([removed_views[i] for i, _ in pairs], dtype=bool).reshape(len(pairs))
    return dict(removed_pairs=removed_pairs, removed_views=removed_views, component=np.where(named, root, -1).astype(np.int32))


# --------------------------------------------------------------------------------------------------------- scenes
def relative_rotation(orient, a, b):
    """rotation_2 of the pair listed (a, b): R_b R_a' (filter_view_graph_cycles_by_rotation_test.cc:66-76)."""
    Ra, Rb = aa_to_R(orient[a][None])[0], aa_to_R(orient[b][None])[0]
    return R_to_aa((Rb @ Ra.T)[None])[0]


def _noisy(rng, rot, sigma_deg):
    """rot composed with a small rotation whose angle-axis components are normal with sigma_deg degrees each."""
    axis = math.radians(sigma_deg) * rng.standard_normal(3)
    return R_to_aa((aa_to_R(axis[None])[0] @ aa_to_R(rot[None])[0])[None])[0]


def _finish(name, n, pairs, rot, thresholds, **extra):
    pairs = np.ascontiguousarray(np.array(pairs, dtype=np.int32).reshape(-1, 2))
    rot = np.ascontiguousarray(np.array(rot, dtype=np.float64).reshape(-1, 3))
    errors = loop_errors(n, pairs, rot)
    ref = {t: cycle_filter(n, pairs, rot, t, errors) for t in thresholds}
    for t in thresholds:
        m = ref[t]["min_loop_error_degrees"]
        gap = np.abs(m[np.isfinite(m)] - t)
        assert gap.size == 0 or gap.min() >= MARGIN, (name, t, gap.min())
    return dict(name=name, n=n, pairs=pairs, rotation_2=rot, thresholds=tuple(thresholds), ref=ref, **extra)


@functools.lru_cache(maxsize=None)
def reference_scene(num_invalid, num_views=10, num_valid=30, seed=57):
    """filter_view_graph_cycles_by_rotation_test.cc:58-161 (numpy's generator in the reference's place): orientations
    uniform in [-1, 1]^3 with view 0 at zero, the skeleton (i - 1, i) and (i - 2, i), random valid pairs up to num_valid,
    then num_invalid further pairs with a random rotation_2.  Threshold 4 degrees (:151).  The reference's test holds
    only when every random valid pair happens to lie in a triangle of valid pairs; the seed is one where it does."""
    rng = np.random.default_rng(seed)
    n = num_views
    orient = rng.uniform(-1.0, 1.0, size=(n, 3))
    orient[0] = 0.0
    pairs = []
    for i in range(1, n):
        pairs.append((i - 1, i))
        if i >= 2:
            pairs.append((i - 2, i))
    seen = set(pairs)
    while len(pairs) < num_valid:
        a, b = (int(v) for v in rng.permutation(n)[:2])
        if a > b or (a, b) in seen:
            continue
        seen.add((a, b))
        pairs.append((a, b))
    rot = [relative_rotation(orient, a, b) for a, b in pairs]
    while len(pairs) < num_valid + num_invalid:
        a, b = sorted(int(v) for v in rng.integers(0, n, size=2))
        if a == b or (a, b) in seen:
            continue
        seen.add((a, b))
        pairs.append((a, b))
        rot.append(rng.uniform(-1.0, 1.0, size=3))
    bad = np.arange(len(pairs)) >= num_valid
    return _finish(f"reference-{num_invalid}", n, pairs, rot, (4.0,), bad=bad)


@functools.lru_cache(maxsize=None)
def hub_scene(spokes=200, seed=7):
    """View 0 joined to `spokes` others, which form a ring: 2 x spokes pairs, spokes triangles, and a hub list longer than
    three wavefront strides.  Every third pair is stored descending; 1.5 degrees of noise per pair; threshold 4."""
    rng = np.random.default_rng(seed)
    n = spokes + 1
    orient = rng.uniform(-1.0, 1.0, size=(n, 3))
    asc = [(0, i) for i in range(1, n)] + [(i, i + 1) for i in range(1, spokes)] + [(1, spokes)]
    pairs, rot = [], []
    for e, (a, b) in enumerate(asc):
        if e % 3 == 2:
            a, b = b, a
        pairs.append((a, b))
        rot.append(_noisy(rng, relative_rotation(orient, a, b), 1.5))
    return _finish("hub", n, pairs, rot, (4.0,))


DENSE_BULK_THRESHOLD = 1.0   # about the median of the good pairs' minima: both outcomes occur among them


@functools.lru_cache(maxsize=None)
def dense_scene(num_views=120, num_pairs=3000, num_bad=300, seed=12):
    """Random pairs in shuffled order, every fifth stored descending; num_bad of them with a random rotation_2, the rest
    with 1 degree of noise.  Thresholds 4 and DENSE_BULK_THRESHOLD."""
    rng = np.random.default_rng(seed)
    n = num_views
    orient = rng.uniform(-1.0, 1.0, size=(n, 3))
    every = [(a, b) for a in range(n) for b in range(a + 1, n)]
    chosen = [every[k] for k in rng.permutation(len(every))[:num_pairs]]   # a random subset in random order
    bad = np.zeros(num_pairs, dtype=bool)
    bad[rng.permutation(num_pairs)[:num_bad]] = True
    pairs, rot = [], []
    for e, (a, b) in enumerate(chosen):
        if e % 5 == 4:
            a, b = b, a
        pairs.append((a, b))
        rot.append(rng.uniform(-1.0, 1.0, size=3) if bad[e] else _noisy(rng, relative_rotation(orient, a, b), 1.0))
    return _finish("dense", n, pairs, rot, (4.0, DENSE_BULK_THRESHOLD), bad=bad)


def exact_rotations(n, pairs, seed=3):
    orient = np.random.default_rng(seed).uniform(-1.0, 1.0, size=(n, 3))
    return [relative_rotation(orient, a, b) for a, b in pairs]


@functools.lru_cache(maxsize=None)
def edge_scenes():
    """name -> scene, a few pairs each; tests/test_view_graph_pruning.py writes their answers out by hand."""
    s = {}

    def add(name, n, pairs, rot=None, thresholds=(4.0,)):
        s[name] = _finish(name, n, pairs, exact_rotations(n, pairs) if rot is None else rot, thresholds)

    add("path", 4, [(0, 1), (1, 2), (2, 3)])
    add("star", 4, [(0, 1), (0, 2), (0, 3)])
    add("four-cycle", 4, [(0, 1), (1, 2), (2, 3), (0, 3)])
    add("exact-triangle", 3, [(0, 1), (0, 2), (1, 2)])
    # loop = R_12 R_01 R_02' = a half-turn about x: the trace of the loop matrix is -1
    add("half-turn", 3, [(0, 1), (0, 2), (1, 2)], rot=[(0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (math.pi, 0.0, 0.0)],
        thresholds=(4.0, 181.0))
    # (0, 1) carries a NaN and lies in the triangles (0, 1, 2) and (0, 1, 3); the triangles (0, 2, 3) and (1, 2, 3) are sound
    pairs = [(0, 1), (0, 2), (1, 2), (0, 3), (1, 3), (2, 3)]
    rot = exact_rotations(4, pairs)
    rot[0] = np.array([np.nan, 0.1, 0.2])
    add("nan-pair", 4, pairs, rot=rot)
    add("unnamed-views", 8, [(1, 4), (4, 6), (1, 6)])                                # views 0, 2, 3, 5, 7 are named by no pair
    add("equal-components", 6, [(1, 3), (3, 5), (1, 5), (0, 2), (2, 4), (0, 4)])   # {1, 3, 5} is listed first, {0, 2, 4} stays
    add("small-component", 5, [(0, 1), (2, 3), (3, 4), (2, 4)])                      # {0, 1} goes, the triangle stays
    return s


def all_scenes():
    return [reference_scene(0), reference_scene(5), reference_scene(15), hub_scene(), dense_scene()] + list(edge_scenes().values())
