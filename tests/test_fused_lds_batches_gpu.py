"""GPU: k_lin_schur / k_backsub_runs where their look-ahead and paired LDS reads can go wrong (csrc/ba_fused.hip).

Phase S reads the mask word and the slot bytes of a step one step ahead (past the last track of a sub-chunk on the last
step, at an index clamped into the tables), the sub-chunk's track count comes from a scalar load issued a phase earlier, and
the track sums of phase L and of the back-substitution take two track positions per trip.  Every sum keeps its operands and
its order, so the results are those of the one-at-a-time loops; the scenes below sit on the places where a pair has a
remainder or a look-ahead leaves the tables' used part, and on every shape of the walk the look-ahead strides over:

  dP (track slices per wave: the stride of the walk is 4 x dP slots) 1, 2, 3, 4, 6, 10;
  unequal slices (slots that are not dense: a slot without a track must match no target), with a constant camera and
      constant points;
  wave groups G = 2 and G = 4 (stride 2 and 1, the lanes of a target spread over the waves of a group);
  a sub-chunk with fewer tracks than one stride of the walk (4 x PS), and one whose track count is no multiple of it;
  runs of one sub-chunk and a run of several (both parities of the mask tables);
  tracks of 1, 2, 3 and 10 observations side by side in the wave tiles (the track sums take two positions per trip);
  last tiles with fewer than 64 observations (every scene).

Every shape is read back from the THEIA_HIP_PLAN_STATS dump, so a scene cannot pass on another shape.  Per scene: the
reduced camera system against the oracle (1e-10 relative, the bound of test_fused_plan_shapes_gpu.py), two calls
bit-identical, a five-iteration LM trace against the oracle (same accept pattern, cost within 1e-9).
scripts/dump_fused_scenes.py dumps the same scenes for a byte comparison of two builds of the library."""
import json

import numpy as np
import pytest

from pytheiasfm_amd import _capi as capi, ba, synth
from tests import oracle_lib as ol
from tests.test_fused_plan_shapes_gpu import SCENES as SHAPE_SCENES

pytestmark = pytest.mark.gpu

FULL7 = list(range(7))


def _scene(nvar, patterns, ntracks, nconst=0, const_every=0, run_obs=None):
    return dict(nvar=nvar, patterns=patterns, ntracks=ntracks, nconst=nconst, const_every=const_every, run_obs=run_obs)


# name -> scene.  nconst: constant cameras behind the variable ones; const_every: every k-th track also sees the first of them
# (the patterns may name them directly as well) and every 11th point from the 6th is constant; run_obs: THEIA_HIP_FUSED_RUN_OBS.
SCENES = {
    "dP10": _scene(3, [[0, 1, 2]], 300),
    "dP10_short": _scene(3, [[0, 1, 2]], 30),                     # one sub-chunk of 30 tracks: fewer than the stride of 40
    "dP6": _scene(4, [[0, 1, 2, 3]], 300),
    "dP4": _scene(5, [[0, 1, 2, 3, 4]], 300),
    "dP4_short": _scene(5, [[0, 1, 2, 3, 4]], 37),                # one sub-chunk of 37 tracks: two strides of 16 and 5 more
    "dP4_long_run": _scene(5, [[0, 1, 2, 3, 4]], 300, run_obs=2048),   # one run of several sub-chunks
    "dP3": _scene(6, [[0, 1, 2, 3, 4, 5]], 300),
    "dP2": _scene(7, [FULL7], 300),
    "dP1": _scene(9, [FULL7, [0, 1, 2, 3, 4, 7, 8]], 300),
    "unequal": _scene(*SHAPE_SCENES[17], 300, nconst=1, const_every=3),
    "G2": _scene(*SHAPE_SCENES[65], 300, nconst=1, const_every=3),
    "G4": _scene(*SHAPE_SCENES[129], 300),
    "lengths": _scene(7, [[0], [0, 1], [0, 1, 2], FULL7 + [7, 8, 9]], 300, nconst=3, const_every=0),
}


def build_scene(name):
    sc = SCENES[name]
    nvar, nv, nt = sc["nvar"], sc["nvar"] + sc["nconst"], sc["ntracks"]
    seed = 0x1D5B0000 + sorted(SCENES).index(name)
    base, cam_gt, pts_gt = synth.synth_ba_v1(nv, nt, seed=seed, mixed_models=True, return_truth=True)
    tracks = [list(sc["patterns"][k % len(sc["patterns"])]) for k in range(nt)]
    cam_const = point_const = None
    if sc["nconst"]:
        cam_const = np.zeros(nv, np.uint8); cam_const[nvar:] = 3
        point_const = np.zeros(nt, np.uint8); point_const[5::11] = 1
        if sc["const_every"]:
            for k in range(0, nt, sc["const_every"]):
                tracks[k] = tracks[k] + [nvar]
    obs_pt = np.repeat(np.arange(nt), [len(t) for t in tracks]).astype(np.int32)
    obs_cam = np.concatenate(tracks).astype(np.int32)
    uv = np.zeros((len(obs_pt), 2))
    for m in np.unique(base.group_model):
        mm = base.group_model[base.cam_group[obs_cam]] == m
        uv[mm], ok = synth.project(m, base.intrinsics[base.cam_group[obs_cam[mm]]], cam_gt[obs_cam[mm]], pts_gt[obs_pt[mm]])
        assert ok.all()
    uv += 0.5 * np.random.default_rng(seed).standard_normal(uv.shape)
    return capi.FlatProblem(base.cam_ext, base.intrinsics, base.group_model, base.cam_group, base.points, uv, obs_cam, obs_pt,
                            cam_const=cam_const, point_const=point_const)


def check_shape(name, plan, p):
    """The runs of the scene's plan have the shape the scene is there for."""
    col = {c: k for k, c in enumerate(plan["run_columns"])}
    rows = [{c: r[k] for c, k in col.items()} for r in plan["run_rows"]]
    assert rows
    ps_of = {"dP10": 10, "dP10_short": 10, "dP6": 6, "dP4": 4, "dP4_short": 4, "dP4_long_run": 4, "dP3": 3, "dP2": 2, "dP1": 1}
    if name in ps_of:   # equal slices, one wave per slice row, PS slices per wave
        assert all(r["G"] == 1 and r["PS"] == ps_of[name] and not r["unequal_slices"] for r in rows), rows
    stride = 4 * rows[0]["PS"]
    if name == "dP10_short":
        assert len(rows) == 1 and rows[0]["tiles"] <= 4 and rows[0]["tracks"] == 30 < stride
    if name == "dP4_short":
        assert len(rows) == 1 and rows[0]["tiles"] <= 4 and rows[0]["tracks"] == 37 and 37 > stride and 37 % stride
    if name == "dP4_long_run":
        assert len(rows) == 1 and rows[0]["tiles"] > 8
    if name == "unequal":
        assert all(r["G"] == 1 for r in rows) and any(r["unequal_slices"] for r in rows), rows
    if name == "G2":
        assert sum(r["G"] == 2 for r in rows) >= len(rows) - 1, rows
    if name == "G4":
        assert sum(r["G"] == 4 for r in rows) >= len(rows) - 1, rows
    if name == "lengths":   # one class (at most seven variable cameras per track): the four lengths alternate inside every tile
        assert all(r["G"] == 1 for r in rows), rows
        # (a constant point seen by a constant camera is a fixed residual block: evaluated once, not part of the plan)
        nfixed = int(np.sum((p.cam_const[p.obs_cam] != 0) & (p.point_const[p.obs_pt] != 0)))
        assert sum(r["observations"] for r in rows) == 75 * (1 + 2 + 3 + 10) - nfixed
    assert any(r["observations"] < 64 * r["tiles"] for r in rows)   # tiles with fewer than 64 observations


def rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


@pytest.mark.parametrize("name", sorted(SCENES))
def test_batched_lds_reads_keep_the_sums(name, tmp_path, monkeypatch):
    p = build_scene(name)
    dump = tmp_path / "plan.json"
    monkeypatch.setenv("THEIA_HIP_PLAN_STATS", str(dump))
    if SCENES[name]["run_obs"]:
        monkeypatch.setenv("THEIA_HIP_FUSED_RUN_OBS", str(SCENES[name]["run_obs"]))
    o, oo = ba.default_options(), ol.default_options()
    with ba.BaHandle(p.copy(), o) as h:
        S1, r1 = h.reduced_system(1e4)
        S2, r2 = h.reduced_system(1e4)
    monkeypatch.delenv("THEIA_HIP_PLAN_STATS")
    check_shape(name, json.loads(dump.read_text()), p)
    # 1, 2: the reduced camera system
    So, ro = ol.reduced_system(p, oo, 1e4)
    assert S1.shape == So.shape
    print(name, "reduced system rel", rel(S1, So), rel(r1, ro))
    assert rel(S1, So) <= 1e-10 and rel(r1, ro) <= 1e-10
    assert np.array_equal(S1, S2) and np.array_equal(r1, r2)
    # 3: five LM iterations
    o.max_num_iterations = 5; oo.max_num_iterations = 5
    pg, po = p.copy(), p.copy()
    s, tr = ba.solve(pg, o)
    so, tro = ol.solve(po, oo)
    assert tr.size == tro.size and tr.size >= 3
    assert np.array_equal(tr.accepted[: tr.size], tro.accepted[: tro.size])
    print(name, "trace cost rel", rel(tr.cost[: tr.size], tro.cost[: tro.size]))
    assert rel(tr.cost[: tr.size], tro.cost[: tro.size]) <= 1e-9
