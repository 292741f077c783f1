"""Times theia_hip_robust_rotation_averaging (RobustRotationEstimator, ROBUST_L1L2) on synthetic view graphs:
1 000 views / 40 000 pairs and 5 000 views / 250 000 pairs, 2 degrees of noise, 10 % outlier edges, initial orientations
chained along the spanning chain (tests/rotation_scenes.py).  One warm-up call per graph, then one timed call.  At 1 000
views the numpy restatement (tests/rotation_averaging_ref.py) runs as well: its CPU time and the largest angle between its
orientations and the device's.  Prints one JSON line."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pytheiasfm_amd import global_pose  # noqa: E402
from tests import rotation_averaging_ref as ref  # noqa: E402
from tests import rotation_scenes as rs  # noqa: E402


def main():
    out = {}
    for n, pairs in ((1000, 40000), (5000, 250000)):
        s = rs.make_scene(n, pairs, 2.0, 0.1, seed=1)
        global_pose.robust_rotation_averaging(s["init"], s["edges"], s["rel"])   # warm-up
        t0 = time.perf_counter()
        rc, got, summ = global_pose.robust_rotation_averaging(s["init"], s["edges"], s["rel"])
        total = 1e3 * (time.perf_counter() - t0)
        row = dict(rc=rc, total_ms=round(total, 2), setup_ms=round(summ.setup_ms, 2), l1_ms=round(summ.l1_ms, 2),
                   irls_ms=round(summ.irls_ms, 2), l1_iterations=summ.l1_iterations, admm_iterations=summ.admm_iterations,
                   irls_iterations=summ.irls_iterations, gt_max_err_deg=round(float(rs.aligned_errors_deg(got, s["gt"]).max()), 4))
        if n == 1000:
            r = ref.robust_rotation_averaging(s["init"], s["edges"], s["rel"])
            row.update(restatement_cpu_ms=round(r["cpu_ms"], 1), max_dev_rad=float(rs.angle_between(got, r["orientations"]).max()),
                       restatement_counts=[r["l1_iterations"], r["admm_iterations"], r["irls_iterations"]])
        out[f"{n}x{pairs}"] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
