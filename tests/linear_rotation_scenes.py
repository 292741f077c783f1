"""Scenes for the LINEAR rotation estimator: the view graphs of tests/rotation_scenes.py (robust_rotation_estimator_test.cc's
generator, which linear_rotation_estimator_test.cc shares) and a ring of cameras whose absolute angles reach 180 degrees
while the relative ones stay small.  scene(name) builds a scene once with its eigh reference and its step-by-step
restatement (tests/linear_rotation_ref.py); nothing that it returns may be modified."""
import functools

import numpy as np

from tests import linear_rotation_ref as ref
from tests import rotation_scenes as rs
from tests.rotation_averaging_ref import aa_to_R, R_to_aa


def make_ring(num_views, noise_deg=0.0, seed=0):
    """`num_views` views turned about y in steps of 360 / num_views degrees; edges to the next two neighbours with
    wrap-around; R_ij = N R_j R_i^T with N a rotation by `noise_deg` about a random axis."""
    rng = np.random.default_rng(seed)
    n = int(num_views)
    gt = np.zeros((n, 3))
    gt[:, 1] = np.radians(360.0 / n) * np.arange(n)
    Rgt = aa_to_R(gt)
    edges = np.array([(i, (i + s) % n) for i in range(n) for s in (1, 2)], dtype=np.int32)
    axis = rng.uniform(-1.0, 1.0, size=(len(edges), 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    N = aa_to_R(np.radians(noise_deg) * axis)
    rel = R_to_aa(N @ Rgt[edges[:, 1]] @ np.transpose(Rgt[edges[:, 0]], (0, 2, 1)))
    return dict(n=n, edges=edges, rel=rel, gt=gt)


# name: (views, pairs, noise in degrees, seed, outlier fraction, duplicated = reversed edges)
GRAPHS = {
    "pair": (2, 1, 1.0, 1, 0.0, 0),
    "tiny0": (4, 6, 0.0, 1, 0.0, 0),
    "tiny1": (4, 6, 1.0, 1, 0.0, 0),
    "v21": (21, 60, 2.0, 2, 0.0, 0),      # n3 = 63: one side of the factorisation's 64-column tile edge
    "v22": (22, 60, 2.0, 2, 0.0, 0),      # n3 = 66: the other side
    "v43": (43, 150, 0.0, 3, 0.0, 0),     # n3 = 129, noise-free
    "v100": (100, 800, 5.0, 4, 0.0, 0),
    "v60dup": (60, 500, 2.0, 1, 0.0, 25),
    "v300out": (300, 3000, 2.0, 1, 0.1, 0),   # the slow-converging case
    "v700": (700, 6000, 2.0, 6, 0.0, 0),      # n3 = 2100: several workgroups in every per-row kernel
}
RINGS = {"ring24": (24, 1.0, 5), "ring24_0": (24, 0.0, 5)}
SCENES = tuple(GRAPHS) + tuple(RINGS)
NOISE_FREE = ("tiny0", "v43", "ring24_0")
# aligned error against the ground truth, degrees: the reference test's kTolerance on noise-free input and its own
# bounds for the two noisy scenes it runs (linear_rotation_estimator_test.cc)
GT_BOUND_DEG = {"tiny0": 1e-6, "v43": 1e-6, "ring24_0": 1e-6, "tiny1": 2.0, "v100": 5.0}


def graph(name):
    """The scene alone: dict(n, edges, rel, gt)."""
    if name in RINGS:
        n, noise, seed = RINGS[name]
        return make_ring(n, noise, seed)
    n, pairs, noise, seed, outliers, dup = GRAPHS[name]
    s = rs.make_scene(n, pairs, noise, outliers, seed=seed)
    if dup:
        s = rs.with_duplicates(s, dup, dup, seed=seed)
    return s


@functools.lru_cache(maxsize=None)
def scene(name):
    """(scene, eigh reference, step-by-step restatement), computed once."""
    s = graph(name)
    return s, ref.reference(s["n"], s["edges"], s["rel"]), ref.device_steps(s["n"], s["edges"], s["rel"])


def connected(num_views, edges):
    """Whether the views that have edges form one connected graph."""
    views, idx = ref.system_views(num_views, edges)
    parent = list(range(len(views)))

    def root(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v
    for i, j in np.asarray(edges).reshape(-1, 2):
        a, b = root(idx[i]), root(idx[j])
        parent[max(a, b)] = min(a, b)
    return len({root(v) for v in range(len(views))}) == 1
