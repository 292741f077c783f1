"""GPU: the fused BA plan on and just past every shape boundary of k_lin_schur's phase S (csrc/ba_plan.hip, csrc/ba_fused.hip).

A run with ntgt target blocks is served by PS = 10 / 6 / 4 / 3 / 2 / 1 track slices per wave (ntgt <= 6 / 10 / 16 / 21 / 32 / 64),
by a group of two waves up to 128 and of four above; inside a one-wave run the slices may be unequal (a narrow slice owns a
prefix of the targets and takes the tracks that need no more).  Every scene here is built so that its runs carry exactly the
target count named in its id -- all tracks start at camera 0, their camera sets are a short cycle of patterns whose union has
that many co-visible pairs -- and the count is read back from the THEIA_HIP_PLAN_STATS dump, so a scene cannot pass on
another shape.  The scenes of 64 targets and more need 11 / 16 / 17 variable cameras (W (W + 1) / 2 >= ntgt).

No cut rule was added with the unequal slices (the run construction already closes a run whose packing level would
drop), so there is no scene for one.  Every scene is ONE (first camera, class) group -- all tracks start at camera 0 and
have at most seven cameras -- cut into several runs by the observation cap: the test asserts that, and that all of the
runs but at most the last carry the target count (a cycle of patterns is shorter than the 64 observations after which
the packing level is held, so no run is closed on the way up).

Per scene: the reduced camera system against the oracle (1e-10 relative, the bound of test_ba_gpu.py), two calls bit-identical,
a five-iteration LM trace against the oracle (same accept pattern, cost within 1e-9), and the same problem with its
observations shuffled between the tracks (the order inside every track kept: it is the summation order of the track's own
sums) on one host thread: bit-identical parameters."""
import json

import numpy as np
import pytest

from pytheiasfm_amd import _capi as capi, ba, synth
from tests import oracle_lib as ol

pytestmark = pytest.mark.gpu


def rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def clique_patterns(m, forbidden, size=6):
    """Camera sets {0} + clique (at most `size` of the cameras 1 .. m) whose union covers every pair of 1 .. m but the forbidden ones."""
    forb = {frozenset(e) for e in forbidden}
    todo = [(i, j) for j in range(1, m + 1) for i in range(j + 1, m + 1) if frozenset((i, j)) not in forb]
    left = set(map(frozenset, todo))
    out = []
    for i, j in todo:
        if frozenset((i, j)) not in left:
            continue
        cl = [j, i]
        while len(cl) < size:
            best, gain = None, 0
            for v in range(1, m + 1):
                if v in cl or any(frozenset((v, c)) in forb for c in cl):
                    continue
                g = sum(frozenset((v, c)) in left for c in cl)
                if g > gain:
                    best, gain = v, g
            if best is None:
                break
            cl.append(best)
        left -= {frozenset((a, b)) for a in cl for b in cl if a != b}
        out.append([0] + sorted(cl))
    return out


# target count -> (variable cameras, camera-set patterns)
SCENES = {
    8: (4, [[0, 1], [0, 2, 3], [0, 2], [0, 3]]),
    9: (5, [[0, 1], [0, 2], [0, 3], [0, 4]]),
    16: (7, [[0, 1, 2], [0, 3, 4], [0, 5, 6], [0, 1], [0, 5]]),
    17: (7, [[0, 1, 2], [0, 3, 4], [0, 5, 6], [0, 2, 3], [0, 1]]),
    21: (7, [[0, 1, 2, 3, 4], [0, 5, 6], [0, 4, 5], [0, 1], [0, 1, 2], [0, 3]]),
    22: (7, [[0, 1, 2, 3, 4], [0, 5, 6], [0, 4, 5], [0, 4, 6], [0, 1], [0, 1, 2]]),
    32: (9, [[0, 1, 2, 3, 4, 5, 6], [0, 7], [0, 8], [0, 1, 2], [0, 1], [0, 1, 2, 3]]),
    33: (9, [[0, 1, 2, 3, 4, 5, 6], [0, 7, 8], [0, 1, 2], [0, 1], [0, 1, 2, 3]]),
    64: (11, clique_patterns(10, [(1, 2), (3, 4)])),
    65: (11, clique_patterns(10, [(1, 2)])),
    128: (16, clique_patterns(15, [(1, 2), (3, 4), (5, 6), (7, 8), (9, 10), (11, 12), (13, 14), (1, 15)])),
    129: (17, clique_patterns(16, [(1, 2), (3, 4), (5, 6), (7, 8), (9, 10), (11, 12), (13, 14), (15, 16), (1, 3), (2, 4),
                                   (5, 7), (6, 8), (9, 11), (10, 12), (13, 15), (14, 16), (1, 4), (2, 3), (5, 8), (6, 7),
                                   (9, 12), (10, 11), (13, 16), (14, 15)])),
}
# the scenes with a constant camera (seen by every third track, not a target) and constant points
WITH_CONSTANTS = (17, 33, 65)
# the scenes whose runs must come out with unequal slices (short and long tracks in a run of one wave per slice row)
UNEQUAL = (16, 17, 21, 22, 32, 33)
NTRACKS = 300


def pairs_of(patterns):
    return len({(max(a, b), min(a, b)) for p in patterns for a in p for b in p})


def build_scene(target):
    nvar, patterns = SCENES[target]
    assert pairs_of(patterns) == target, (target, pairs_of(patterns))
    nv = nvar + (1 if target in WITH_CONSTANTS else 0)
    base, cam_gt, pts_gt = synth.synth_ba_v1(nv, NTRACKS, seed=0x5A9E0000 + target, mixed_models=True, return_truth=True)
    tracks = [list(patterns[k % len(patterns)]) for k in range(NTRACKS)]
    cam_const = point_const = None
    if target in WITH_CONSTANTS:
        cam_const = np.zeros(nv, np.uint8); cam_const[nvar] = 3
        point_const = np.zeros(NTRACKS, np.uint8); point_const[5::11] = 1
        for k in range(0, NTRACKS, 3):
            tracks[k] = tracks[k] + [nvar]
    obs_pt = np.repeat(np.arange(NTRACKS), [len(t) for t in tracks]).astype(np.int32)
    obs_cam = np.concatenate(tracks).astype(np.int32)
    uv = np.zeros((len(obs_pt), 2))
    for m in np.unique(base.group_model):
        mm = base.group_model[base.cam_group[obs_cam]] == m
        uv[mm], ok = synth.project(m, base.intrinsics[base.cam_group[obs_cam[mm]]], cam_gt[obs_cam[mm]], pts_gt[obs_pt[mm]])
        assert ok.all()
    uv += 0.5 * np.random.default_rng(target).standard_normal(uv.shape)
    return capi.FlatProblem(base.cam_ext, base.intrinsics, base.group_model, base.cam_group, base.points, uv, obs_cam, obs_pt,
                            cam_const=cam_const, point_const=point_const)


def shuffled_between_tracks(p, seed):
    """The observations in a random order that keeps the order inside every track."""
    key = np.random.default_rng(seed).random(len(p.obs_pt))
    by_track = np.lexsort((np.arange(len(key)), p.obs_pt))           # track by track, input order inside
    sorted_keys = key[np.lexsort((key, p.obs_pt))]                   # every track's keys, ascending
    pos = np.empty(len(key)); pos[by_track] = sorted_keys            # k-th observation of a track gets its k-th smallest key
    order = np.argsort(pos, kind="stable")
    return capi.FlatProblem(p.cam_ext.copy(), p.intrinsics.copy(), p.group_model, p.cam_group, p.points.copy(), p.obs_uv[order],
                            p.obs_cam[order], p.obs_pt[order], p.cam_const, p.group_const, p.point_const)


@pytest.mark.parametrize("target", sorted(SCENES))
def test_runs_on_and_past_every_shape_boundary(target, tmp_path, monkeypatch):
    p = build_scene(target)
    dump = tmp_path / "plan.json"
    monkeypatch.setenv("THEIA_HIP_PLAN_STATS", str(dump))
    o, oo = ba.default_options(), ol.default_options()
    with ba.BaHandle(p.copy(), o) as h:
        S1, r1 = h.reduced_system(1e4)
        S2, r2 = h.reduced_system(1e4)
    monkeypatch.delenv("THEIA_HIP_PLAN_STATS")
    plan = json.loads(dump.read_text())
    col = {name: k for k, name in enumerate(plan["run_columns"])}
    rows = plan["run_rows"]
    ntgt = [r[col["ntgt"]] for r in rows]
    assert len(rows) >= 2 and sum(n == target for n in ntgt) >= len(rows) - 1 and ntgt[0] == target, ntgt   # one group, cut by the cap
    full = [r for r in rows if r[col["ntgt"]] == target]
    want_g = 1 if target <= 33 else (2 if target <= 128 else 4)   # (the scenes of 64 and more have 11 or more cameras: 6 W > 64)
    assert all(r[col["G"]] == want_g for r in full), [(r[col["G"]], r[col["PS"]]) for r in full]
    if target <= 33:
        equal_ps = next(c for c in (10, 6, 4, 3, 2, 1) if 64 // c >= target)
        assert all(r[col["unequal_slices"]] or r[col["PS"]] == equal_ps for r in full)
    if target in UNEQUAL:   # mixed track lengths in a one-wave run: narrower slices beside the full one
        assert any(r[col["unequal_slices"]] for r in full)
    for r in rows:
        assert 64 * r[col["steps_issued"]] == r[col["lanes_useful"]] + r[col["lanes_idle_shape"]] + r[col["lanes_idle_sparsity"]]
    # (a constant point seen by the constant camera is a fixed residual block: evaluated once, not part of the plan)
    nfixed = 0 if p.cam_const is None else int(np.sum((p.cam_const[p.obs_cam] != 0) & (p.point_const[p.obs_pt] != 0)))
    assert sum(r[col["observations"]] for r in rows) == plan["total"]["observations"] == len(p.obs_pt) - nfixed
    # 1, 2: the reduced camera system
    So, ro = ol.reduced_system(p, oo, 1e4)
    assert S1.shape == So.shape
    assert rel(S1, So) <= 1e-10 and rel(r1, ro) <= 1e-10
    assert np.array_equal(S1, S2) and np.array_equal(r1, r2)
    # 3: five LM iterations
    o.max_num_iterations = 5; oo.max_num_iterations = 5
    pg, po = p.copy(), p.copy()
    s, tr = ba.solve(pg, o)
    so, tro = ol.solve(po, oo)
    assert tr.size == tro.size and tr.size >= 3
    assert np.array_equal(tr.accepted[: tr.size], tro.accepted[: tro.size])
    assert rel(tr.cost[: tr.size], tro.cost[: tro.size]) <= 1e-9
    # 4: observations shuffled between the tracks, one host thread
    q = shuffled_between_tracks(p, target)
    assert np.any(np.diff(q.obs_pt) < 0)
    monkeypatch.setenv("THEIA_HIP_HOST_THREADS", "1")
    qs, _ = ba.solve(q, o)
    monkeypatch.delenv("THEIA_HIP_HOST_THREADS")
    assert qs.num_iterations == s.num_iterations
    assert np.array_equal(q.cam_ext, pg.cam_ext) and np.array_equal(q.points, pg.points)

