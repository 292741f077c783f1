"""Times theia_hip_ligt_positions (the LiGT position stage, csrc/ligt_positions.hip) at two sizes of synth.ba_config:
C4, 1 000 views / 500 000 tracks / 3.0 M observations (BASELINE's problem), and C2, 200 views / 50 000 tracks.  The
topology is the configuration's (tracks over windows of a ring of cameras, 2 to 10 observations each); the normalised
features are the exact projections hnormalized(R (X - c)) of its points into its cameras, so the positions come back as
s (c - c_held) and the relative error of that fit is reported with the times.  The view pairs of the sign vote are the
ring's neighbours.  One warm-up call per scene, then one timed call: total wall time and the summary's stage times
(set-up = checks, uploads, pair search and the host plan; assembly; factorisation; inverse iteration with the sign vote
and the downloads).  At 200 views the numpy restatement (tests/ligt_positions_ref.py) is timed on the same scene.
Per-launch times come from a run of their own:
  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python scripts/gpu_time_ligt.py
Prints one JSON line."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pytheiasfm_amd import global_pose, synth  # noqa: E402
from tests import ligt_positions_ref as ref  # noqa: E402


def scene(config):
    p = synth.ba_config(config)
    pos, aa = p.cam_ext[:, :3], p.cam_ext[:, 3:6]
    R = synth.angle_axis_to_matrix(aa)
    q = np.einsum("nij,nj->ni", R[p.obs_cam], p.points[p.obs_pt, :3] - pos[p.obs_cam])
    feats = q[:, :2] / q[:, 2:3]
    assert np.all(np.diff(p.obs_pt) >= 0)
    offsets = np.concatenate([[0], np.cumsum(np.bincount(p.obs_pt, minlength=p.points.shape[0]))]).astype(np.int32)
    nv = pos.shape[0]
    edges = np.array([(i, (i + 1) % nv) for i in range(nv)], dtype=np.int32)
    d = pos[edges[:, 1]] - pos[edges[:, 0]]
    rel = np.einsum("nij,nj->ni", R[edges[:, 0]], d / np.linalg.norm(d, axis=1, keepdims=True))
    return dict(aa=aa, pos=pos, offsets=offsets, obs_view=p.obs_cam, feats=feats, edges=edges, rel=rel)


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
        args = (s["aa"], s["offsets"], s["obs_view"], s["feats"], s["edges"], s["rel"])
        global_pose.ligt_positions(*args)   # warm-up
        t0 = time.perf_counter()
        rc, p, est, k, extra = global_pose.ligt_positions(*args, want=("system_index",))
        total = 1e3 * (time.perf_counter() - t0)
        row = dict(rc=rc, views=len(s["aa"]), tracks=len(s["offsets"]) - 1, observations=len(s["obs_view"]),
                   total_ms=round(total, 2), setup_ms=round(k.setup_ms, 2), assemble_ms=round(k.assemble_ms, 2),
                   factor_ms=round(k.factor_ms, 2), eig_ms=round(k.eig_ms, 2), iterations=k.iterations,
                   converged=k.converged, views_in_system=k.num_views_in_system, tracks_used=k.tracks_used,
                   constraints=k.num_constraints, eigenvalue=k.eigenvalue, shift=k.shift, sign_votes=k.sign_votes,
                   flipped=k.flipped)
        if rc == 0:
            scale, err = fit_error(s, p, est, extra["system_index"])
            row.update(scale=scale, relative_error=err)
        if config == "C2" and rc == 0:
            t1 = time.perf_counter()
            r = ref.estimate(*args)
            row.update(restatement_cpu_ms=round(1e3 * (time.perf_counter() - t1), 1),
                       restatement_index_equal=bool(np.array_equal(r["index"], extra["system_index"])),
                       restatement_max_position_difference=float(np.abs(r["positions"] - p).max()))
        out[config] = row
        print(json.dumps({config: row}), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
