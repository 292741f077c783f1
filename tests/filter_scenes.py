"""Scenes for the two view-graph filters.

reference_translation_scene / line_scene restate the scenes of filter_view_pairs_from_relative_translation_test.cc:58-203
and reference_orientation_scene those of filter_view_pairs_from_orientation_test.cc:57-170 (numpy's generator in place
of the reference's: the scenes are built the same way, they are not the same numbers): orientations and positions
uniform in [-1, 1]^3 with view 0 at zero, the chain pairs (i - 1, i), random extra valid pairs (first id smaller),
rotation_2 = R_2 R_1', position_2 = R_1 (c_2 - c_1) / |c_2 - c_1|; an invalid pair gets rotation_2 + (1, 1, 1) and a random
unit position_2.  The larger scenes come from tests/position_scenes.py, the ones the position stage is tested on."""
import numpy as np

from tests import position_scenes as ps
from tests.rotation_averaging_ref import aa_to_R, R_to_aa


LINE_SEED = 199   # the reference's own LineTest seed: the restatement removes exactly (0, 3) under it (test_view_pair_filters.py)


def _two_view(orient, pos, a, b):
    R1, R2 = aa_to_R(orient[a][None])[0], aa_to_R(orient[b][None])[0]
    rot = R_to_aa((R2 @ R1.T)[None])[0]
    d = pos[b] - pos[a]
    return rot, R1 @ (d / np.linalg.norm(d))


def reference_translation_scene(num_views, num_valid, num_invalid, seed=0, ordered_invalid=True):
    rng = np.random.default_rng(seed)
    n = int(num_views)
    orient = rng.uniform(-1.0, 1.0, size=(n, 3))
    pos = rng.uniform(-1.0, 1.0, size=(n, 3))
    orient[0] = 0.0
    pos[0] = 0.0
    pairs = [(i - 1, i) for i in range(1, n)]
    seen = set(pairs)
    while len(pairs) < num_valid:
        a, b = (int(v) for v in rng.permutation(n)[:2])
        if a > b or (a, b) in seen:
            continue
        seen.add((a, b))
        pairs.append((a, b))
    rot, tr = [], []
    for a, b in pairs:
        r, t = _two_view(orient, pos, a, b)
        rot.append(r)
        tr.append(t)
    valid = len(pairs)
    while len(pairs) < valid + num_invalid:
        a, b = (int(v) for v in rng.integers(0, n, size=2))
        if a == b or (ordered_invalid and a > b) or (a, b) in seen or (b, a) in seen:
            continue
        seen.add((a, b))
        pairs.append((a, b))
        r, _ = _two_view(orient, pos, a, b)
        v = rng.uniform(-1.0, 1.0, size=3)
        rot.append(r + 1.0)
        tr.append(v / np.linalg.norm(v))
    invalid = np.arange(len(pairs)) >= valid
    return dict(n=n, pairs=np.array(pairs, dtype=np.int32).reshape(-1, 2), orientations=orient, positions=pos,
                rotation_2=np.array(rot), position_2=np.array(tr), invalid=invalid, num_valid=valid)


def reference_orientation_scene(num_views, num_valid, num_invalid, seed=0):
    """The orientation test's scenes: an invalid pair may run either way."""
    return reference_translation_scene(num_views, num_valid, num_invalid, seed=seed, ordered_invalid=False)


def line_scene():
    """LineTest (:161-187): four views on the x axis at the identity, the chain, and the pair (0, 3) pointing backwards."""
    orient = np.zeros((4, 3))
    pos = np.array([[float(i), 0.0, 0.0] for i in range(4)])
    pairs = np.array([(0, 1), (1, 2), (2, 3), (0, 3)], dtype=np.int32)
    tr = np.array([[1.0, 0.0, 0.0]] * 3 + [list(np.array([-1.0, -1.0, -1.0]) / np.sqrt(3.0))])
    return dict(n=4, pairs=pairs, orientations=orient, positions=pos, rotation_2=np.zeros((4, 3)), position_2=tr,
                invalid=np.array([False, False, False, True]), num_valid=3)


def position_scene(num_views, num_pairs, noise_deg=2.0, outlier_fraction=0.1, seed=0):
    """A scene of tests/position_scenes.py under this module's names."""
    s = ps.make_scene(num_views, num_pairs, noise_deg, outlier_fraction, seed=seed)
    return dict(n=s["n"], pairs=s["edges"], orientations=s["orientations"], positions=s["gt"], position_2=s["rel"],
                invalid=s["outliers"], num_valid=int((~s["outliers"]).sum()))


def components_scene(sizes=((25, 120), (20, 80), (9, 20)), isolated=6, seed=0):
    """Several connected components and `isolated` views that no pair names, the view indices shuffled so that the
    components interleave and the isolated views sit between them."""
    rng = np.random.default_rng(seed)
    parts = [ps.make_scene(n, p, 2.0, 0.1, seed=seed + 10 * k) for k, (n, p) in enumerate(sizes)]
    total = sum(s["n"] for s in parts) + isolated
    new = rng.permutation(total)
    orient = 0.2 * rng.uniform(-1.0, 1.0, size=(total, 3))
    pos = 10.0 * rng.uniform(-1.0, 1.0, size=(total, 3))
    pairs, tr, base = [], [], 0
    for s in parts:
        ids = new[base:base + s["n"]]
        orient[ids] = s["orientations"]
        pos[ids] = s["gt"]
        pairs.append(ids[s["edges"]])
        tr.append(s["rel"])
        base += s["n"]
    pairs = np.ascontiguousarray(np.concatenate(pairs).astype(np.int32))
    named = np.zeros(total, bool)
    named[pairs.ravel()] = True
    return dict(n=total, pairs=pairs, orientations=orient, positions=pos, position_2=np.concatenate(tr),
                invalid=np.concatenate([s["outliers"] for s in parts]), isolated=np.flatnonzero(~named))


def unit_axes(num_iterations, seed=0):
    """Projection axes to hand in: random unit vectors."""
    v = np.random.default_rng(seed).standard_normal((num_iterations, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)
