"""Times theia_hip_nonlinear_rotations (NonlinearRotationEstimator, NONLINEAR) on synthetic view graphs: 1 000 views /
40 000 pairs and 5 000 views / 250 000 pairs, 2 degrees of noise, chain initialisation (tests/rotation_scenes.py).  One
warm-up call per graph, then one timed call.  Prints one JSON line."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pytheiasfm_amd import global_pose  # noqa: E402
from tests import rotation_scenes as rs  # noqa: E402


def main():
    out = {}
    for n, pairs in ((1000, 40000), (5000, 250000)):
        s = rs.make_scene(n, pairs, 2.0, seed=1)
        global_pose.nonlinear_rotations(s["init"], s["edges"], s["rel"])   # warm-up
        t0 = time.perf_counter()
        rc, got, summ = global_pose.nonlinear_rotations(s["init"], s["edges"], s["rel"])
        total = 1e3 * (time.perf_counter() - t0)
        out[f"{n}x{pairs}"] = dict(rc=rc, total_ms=round(total, 2), solve_ms=round(1e3 * summ.seconds, 2),
                                   iterations=summ.iterations, successful=summ.num_successful_steps,
                                   invalid=summ.num_invalid_steps, termination=summ.termination,
                                   initial_cost=summ.initial_cost, final_cost=summ.final_cost,
                                   init_max_err_deg=round(float(rs.aligned_errors_deg(s["init"], s["gt"]).max()), 4),
                                   gt_max_err_deg=round(float(rs.aligned_errors_deg(got, s["gt"]).max()), 4))
        print(json.dumps({f"{n}x{pairs}": out[f"{n}x{pairs}"]}), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
