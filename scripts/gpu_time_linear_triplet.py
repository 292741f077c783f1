"""Times theia_hip_linear_triplet_positions (the LINEAR_TRIPLET position stage, csrc/linear_positions.hip) at two sizes of
synth.ba_config: C4, 1 000 views / 500 000 tracks / 3.0 M observations (BASELINE's problem), and C2, 200 views / 50 000
tracks.  The topology is the configuration's (tracks over windows of a ring of cameras); the view pairs join every view
to its next NEIGHBOURS views on the ring, so that every window of three is a triangle; rotation_2 = log(R_j R_i'),
position_2 = R_i (c_j - c_i) / |.| and the normalised features are the exact projections, so the positions come back
as s (c - c_held) and the relative error of that fit is reported with the times.  One warm-up call per scene, then one
timed call: total wall time and the summary's stage times (set-up = checks, lists, uploads; triangles; baseline ratios;
the host plan and the assembly; factorisation; inverse iteration with the sign vote and the downloads).  Each figure is
a single sample.  At 200 views the ratio stage of the numpy restatement (tests/linear_triplet_ref.baseline_stage) is
timed on the same scene.  Per-launch times come from a run of their own:
  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python scripts/gpu_time_linear_triplet.py
Prints one JSON line."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pytheiasfm_amd import global_pose, synth  # noqa: E402
from tests import linear_triplet_ref as ref  # noqa: E402

NEIGHBOURS = 8


def log_rotations(R):
    """Angle-axis of rotation matrices [k][3][3] (angles below pi)."""
    c = np.clip((np.trace(R, axis1=1, axis2=2) - 1.0) / 2.0, -1.0, 1.0)
    th = np.arccos(c)
    v = np.stack([R[:, 2, 1] - R[:, 1, 2], R[:, 0, 2] - R[:, 2, 0], R[:, 1, 0] - R[:, 0, 1]], axis=1)
    k = np.where(th < 1e-12, 0.5, th / (2.0 * np.sin(np.where(th < 1e-12, 1.0, th))))
    return k[:, None] * v


def scene(config):
    p = synth.ba_config(config)
    pos, aa = p.cam_ext[:, :3], p.cam_ext[:, 3:6]
    R = synth.angle_axis_to_matrix(aa)
    q = np.einsum("nij,nj->ni", R[p.obs_cam], p.points[p.obs_pt, :3] - pos[p.obs_cam])
    feats = q[:, :2] / q[:, 2:3]
    assert np.all(np.diff(p.obs_pt) >= 0)
    offsets = np.concatenate([[0], np.cumsum(np.bincount(p.obs_pt, minlength=p.points.shape[0]))]).astype(np.int32)
    nv = pos.shape[0]
    pairs = {(min(i, (i + k) % nv), max(i, (i + k) % nv)) for i in range(nv) for k in range(1, NEIGHBOURS + 1)}
    edges = np.array(sorted(pairs), dtype=np.int32)
    i, j = edges[:, 0], edges[:, 1]
    d = pos[j] - pos[i]
    rel = np.einsum("nij,nj->ni", R[i], d / np.linalg.norm(d, axis=1, keepdims=True))
    rot = log_rotations(np.einsum("nij,nkj->nik", R[j], R[i]))
    return dict(aa=aa, pos=pos, offsets=offsets, obs_view=p.obs_cam, feats=feats, edges=edges, rot=rot, rel=rel)


def fit_error(s, positions, estimated, index):
    held = int(np.nonzero(index == -1)[0][0])
    d = (s["pos"] - s["pos"][held])[estimated]
    p = positions[estimated]
    k = float((p * d).sum() / (d * d).sum())
    return k, float(np.linalg.norm(p - k * d, axis=1).max() / np.linalg.norm(k * d))


def main():
    out = {}
    configs = ("C4", "C2")
    if len(sys.argv) > 1:
        configs = tuple(c for c in configs if c in sys.argv[1:])
    for config in configs:
        s = scene(config)
        args = (s["aa"], s["edges"], s["rot"], s["rel"], s["offsets"], s["obs_view"], s["feats"])
        global_pose.linear_triplet_positions(*args)   # warm-up
        t0 = time.perf_counter()
        rc, p, est, k, extra = global_pose.linear_triplet_positions(*args, want=("system_index", "baselines"))
        total = 1e3 * (time.perf_counter() - t0)
        row = dict(rc=rc, views=len(s["aa"]), pairs=len(s["edges"]), tracks=len(s["offsets"]) - 1,
                   observations=len(s["obs_view"]), total_ms=round(total, 2))
        row.update({name: (round(v, 2) if name.endswith("_ms") else v) for name, v in k.as_dict().items()})
        if rc == 0:
            scale, err = fit_error(s, p, est, extra["system_index"])
            row.update(scale=scale, relative_error=err)
        if config == "C2" and rc == 0:
            t1 = time.perf_counter()
            r = ref.baseline_stage(len(s["aa"]), *args[1:])
            row.update(restatement_ratio_stage_cpu_ms=round(1e3 * (time.perf_counter() - t1), 1),
                       restatement_triangles=len(r["triplets"]), restatement_common_tracks=int(r["common"].sum()),
                       restatement_states_equal=bool(np.array_equal(extra["baselines"][:, 0] == 0.0, r["state"] == 1)),
                       restatement_max_relative_baseline_difference=float(
                           np.abs(extra["baselines"][r["state"] == 0, 1:] / r["baselines"][r["state"] == 0, 1:] - 1.0).max()))
        out[config] = row
        print(json.dumps({config: row}), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
