"""Times theia_hip_lud_positions (LeastUnsquaredDeviationPositionEstimator, LEAST_UNSQUARED_DEVIATION) on synthetic
scenes: 1 000 views / 40 000 pairs and 5 000 views / 250 000 pairs, 2 degrees of noise, 10 % outlier directions
(tests/position_scenes.py).  One warm-up call per scene, then one timed call: setup, factor and ADMM ms, iterations and
ms per ADMM iteration.  At 1 000 views the numpy restatement (tests/lud_positions_ref.py, Schur form) runs as well: its
CPU time and the largest deviation of its positions from the device's, relative to the scene's extent.
Prints one JSON line."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pytheiasfm_amd import global_pose  # noqa: E402
from tests import lud_positions_ref as ref  # noqa: E402
from tests import position_scenes as ps  # noqa: E402


def main():
    out = {}
    sizes = ((1000, 40000), (5000, 250000))
    if len(sys.argv) > 1:
        sizes = tuple(s for s in sizes if str(s[0]) in sys.argv[1:])
    for n, pairs in sizes:
        s = ps.make_scene(n, pairs, 2.0, 0.1, seed=1)
        global_pose.lud_positions(s["orientations"], s["edges"], s["rel"])   # warm-up
        t0 = time.perf_counter()
        rc, got, summ = global_pose.lud_positions(s["orientations"], s["edges"], s["rel"])
        total = 1e3 * (time.perf_counter() - t0)
        row = dict(rc=rc, total_ms=round(total, 2), setup_ms=round(summ.setup_ms, 2), factor_ms=round(summ.factor_ms, 2),
                   admm_ms=round(summ.admm_ms, 2), admm_iterations=summ.admm_iterations, converged=summ.converged,
                   ms_per_admm_iteration=round(summ.admm_ms / max(1, summ.admm_iterations), 4),
                   gt_max_err=round(float(ps.aligned_errors(got, s["gt"]).max()), 4))
        if n == 1000:
            r = ref.lud_positions(s["orientations"], s["edges"], s["rel"], form="schur")
            row.update(restatement_cpu_ms=round(r["cpu_ms"], 1), restatement_iterations=r["admm_iterations"],
                       max_dev_rel=float(np.abs(got - r["positions"]).max() / ps.extent(r["positions"])))
        out[f"{n}x{pairs}"] = row
        print(json.dumps({f"{n}x{pairs}": row}), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
