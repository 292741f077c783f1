"""Times theia_hip_pose_graph_sim3 on the GPU: a ring of n nodes with random chords up to E edges, node 0
held, measurements = the ground truth's relative Sim(3) plus 1e-3 noise, the start drifted by 0.02; 1 000 nodes / 5 000 edges
and 2 000 nodes / 20 000 edges.  Every figure is ONE timed call after one untimed call of the same shape; kernel ms are
device events around the call's kernels (summary.kernel_ms), call ms the whole C entry (summary.seconds).
    python scripts/gpu_time_pose_graph_sim3.py"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytheiasfm_amd import alignment as al  # noqa: E402


def graph(n, E, rng):
    ang = 2.0 * np.pi * np.arange(n) / n
    gt = np.stack([4.0 * np.cos(ang), 0.2 * np.sin(3.0 * ang), 4.0 * np.sin(ang), 0.3 * np.sin(ang), ang - np.pi,
                   0.2 * np.cos(ang), 0.1 * np.sin(ang)], axis=1)
    ring = np.stack([np.arange(n), (np.arange(n) + 1) % n], axis=1)
    a = rng.integers(0, n, size=E - n)
    chords = np.stack([a, (a + rng.integers(2, 40, size=E - n)) % n], axis=1)
    edges = np.concatenate([ring, chords]).astype(np.int32)
    z = al.RelativeSim3s(gt, edges) + 1e-3 * rng.standard_normal((E, 7))
    start = gt.copy()
    start[1:] += 0.02 * rng.standard_normal((n - 1, 7))
    fixed = np.zeros(n, dtype=np.uint8)
    fixed[0] = 1
    return start, edges, z, fixed


def timed(n, E, rng):
    start, edges, z, fixed = graph(n, E, rng)
    al.OptimizePoseGraphSim3(start, edges, z, None, fixed)
    _, s = al.OptimizePoseGraphSim3(start, edges, z, None, fixed)
    return dict(kernel_ms=round(s.kernel_ms, 3), call_ms=round(1e3 * s.seconds, 3), iterations=s.iterations,
                successful=s.num_successful_steps, termination=s.termination, initial_cost=s.initial_cost, final_cost=s.final_cost)


def main():
    rng = np.random.default_rng(7)
    for n, E in ((1000, 5000), (2000, 20000)):
        print(f"{n} nodes / {E} edges", json.dumps(timed(n, E, rng)), flush=True)


if __name__ == "__main__":
    main()
