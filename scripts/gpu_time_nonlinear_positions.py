"""Times the NONLINEAR position stage (NonlinearPositionEstimator, theia_hip_nonlinear_positions) on synthetic scenes:
1 000 views / 40 000 pairs and 5 000 views / 250 000 pairs, each with no points and with min_num_points_per_view = 10
over tracks of ten views.  Half a degree of noise on the pairs' directions, view 0 held, the start 0.05 off the truth per
coordinate (EstimateRemainingPositionsInRecon: the random start of EstimatePositions is a different measurement).  One
warm-up call per row, then one timed call.  Prints one JSON line."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pytheiasfm_amd import sfm  # noqa: E402
from pytheiasfm_amd.synth import angle_axis_to_matrix  # noqa: E402
from pytheiasfm_amd.twoview import TwoViewInfo  # noqa: E402


def make_scene(n, num_pairs, seed=1, track_length=10):
    rng = np.random.default_rng(seed)
    gt = rng.normal(0.0, 5.0, (n, 3))
    aa = 0.2 * rng.uniform(-1.0, 1.0, (n, 3))
    R = angle_axis_to_matrix(aa)
    chain = np.column_stack([np.arange(n - 1), np.arange(1, n)])                                # connected, then random pairs
    extra = rng.integers(0, n, (2 * num_pairs, 2))
    extra = np.unique(np.sort(extra[extra[:, 0] != extra[:, 1]], axis=1), axis=0)
    extra = extra[extra[:, 1] != extra[:, 0] + 1]
    extra = extra[rng.permutation(len(extra))[:num_pairs - (n - 1)]]
    e = np.concatenate([chain, extra])
    e = e[rng.permutation(len(e))]
    d = gt[e[:, 1]] - gt[e[:, 0]]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rel = np.einsum("eij,ej->ei", R[e[:, 0]], d) + np.tan(np.radians(0.5)) * rng.normal(0.0, 1.0, d.shape) / np.sqrt(3.0)
    rel /= np.linalg.norm(rel, axis=1, keepdims=True)
    T = 2 * n
    X = np.column_stack([rng.normal(0.0, 5.0, (T, 2)), rng.uniform(40.0, 60.0, T)])
    ov = (rng.integers(0, n, T)[:, None] + np.arange(track_length)[None, :]) % n                 # ten consecutive views
    ot = np.repeat(np.arange(T), track_length)
    ov = ov.reshape(-1)
    p = np.einsum("oij,oj->oi", R[ov], X[ot] - gt[ov])
    r = sfm.Reconstruction()
    r.cam_ext = np.column_stack([gt + rng.normal(0.0, 0.05, gt.shape), aa])
    r.view_estimated = np.ones(n, dtype=bool)
    r.points = np.column_stack([X + rng.normal(0.0, 0.1, X.shape), np.ones(T)])
    r.track_estimated = np.ones(T, dtype=bool)
    r.obs_view, r.obs_track = ov.astype(np.int32), ot.astype(np.int32)
    r.obs_uv = p[:, :2] / p[:, 2:3] + rng.normal(0.0, 1e-3, (len(ov), 2))
    pairs = {}
    for (a, b), t in zip(e, rel):
        info = TwoViewInfo()
        info.position_2 = t
        pairs[(int(a), int(b))] = info
    return r, pairs, gt, e


def main():
    out = {}
    for n, num_pairs in ((1000, 40000), (5000, 250000)):
        r, pairs, gt, e = make_scene(n, num_pairs)
        d_gt = gt[e[:, 1]] - gt[e[:, 0]]
        d_gt /= np.linalg.norm(d_gt, axis=1, keepdims=True)
        for k in (0, 10):
            o = sfm.NonlinearPositionEstimatorOptions()
            o.min_num_points_per_view = k
            est = sfm.NonlinearPositionEstimator(o, r, normalized_features=r.obs_uv)
            est.EstimateRemainingPositionsInRecon([0], range(n), pairs)                        # warm-up
            t0 = time.perf_counter()
            ok, pos = est.EstimateRemainingPositionsInRecon([0], range(n), pairs)
            total = 1e3 * (time.perf_counter() - t0)
            s = est.last_summary
            x = np.array([pos[v] for v in range(n)])
            d = x[e[:, 1]] - x[e[:, 0]]
            d /= np.linalg.norm(d, axis=1, keepdims=True)
            ang = np.degrees(np.arccos(np.clip((d * d_gt).sum(1), -1.0, 1.0)))
            key = f"{n}x{len(e)}_k{k}"
            out[key] = dict(ok=bool(ok), total_ms=round(total, 2), solve_ms=round(1e3 * s.seconds, 2),
                            order=3 * (s.num_views_in_problem + s.num_points_in_problem),
                            points=s.num_points_in_problem, point_edges=s.num_point_edges_in_problem,
                            iterations=s.iterations, successful=s.num_successful_steps, invalid=s.num_invalid_steps,
                            termination=s.termination, initial_cost=s.initial_cost, final_cost=s.final_cost,
                            median_direction_error_deg=round(float(np.median(ang)), 4))
            print(json.dumps({key: out[key]}), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
