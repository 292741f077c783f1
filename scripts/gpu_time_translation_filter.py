"""Times theia_hip_filter_view_pairs_from_relative_translation (the 1DSfM filter, csrc/view_pair_filters.hip) on the two
scenes the other global stages are timed on: 1 000 views / 40 000 pairs and 5 000 views / 250 000 pairs, 2 degrees of
noise, 10 % outlier directions (tests/position_scenes.py), 48 iterations, axes drawn from a seeded generator.  One
warm-up call per scene, then one timed call: total and the host-side stage times (set-up = checks, CSR, allocation and
upload; rotate + project; ordering; weights), microseconds per ordering step (ordering time / views), the steps that
took a source against those that took an arg-max, the route of the per-view state, and how many outlier / inlier pairs
were removed.  At 1 000 views the numpy restatement (tests/translation_filter_ref.py) runs on the device's axes: its
wall time, and whether its verdicts equal the device's.  Per-launch times come from a run of their own:
  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python scripts/gpu_time_translation_filter.py
Prints one JSON line."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pytheiasfm_amd import _capi as capi, global_pose, ransac  # noqa: E402
from tests import position_scenes as ps  # noqa: E402
from tests import translation_filter_ref as ref  # noqa: E402


def main():
    out = {}
    sizes = ((1000, 40000), (5000, 250000))
    if len(sys.argv) > 1:
        sizes = tuple(s for s in sizes if str(s[0]) in sys.argv[1:])
    for n, pairs in sizes:
        s = ps.make_scene(n, pairs, 2.0, 0.1, seed=1)
        st = capi.RngState()
        capi.check(ransac._sig().theia_hip_rng_seed(C.byref(st), 169))
        global_pose.filter_translations_1dsfm(s["orientations"], s["edges"], s["rel"], rng_state=st)   # warm-up
        capi.check(ransac._sig().theia_hip_rng_seed(C.byref(st), 169))
        t0 = time.perf_counter()
        rc, removed, got = global_pose.filter_translations_1dsfm(s["orientations"], s["edges"], s["rel"], rng_state=st,
                                                                 want=("axes", "rotated"))
        total = 1e3 * (time.perf_counter() - t0)
        k = global_pose.translation_filter_last_stats()
        row = dict(rc=rc, total_ms=round(total, 2), setup_ms=round(k["setup_ms"], 2),
                   rotate_project_ms=round(k["rotate_project_ms"], 2), order_ms=round(k["order_ms"], 2),
                   weights_ms=round(k["weights_ms"], 2), us_per_order_step=round(1e3 * k["order_ms"] / n, 3),
                   source_steps=k["source_steps"], argmax_steps=k["argmax_steps"],
                   route="lds" if k["lds_route"] else "global", order_threads=k["order_threads"],
                   removed=int(removed.sum()), outliers=int(s["outliers"].sum()),
                   outliers_removed=int((removed & s["outliers"]).sum()), inliers_removed=int((removed & ~s["outliers"]).sum()))
        if n == 1000:
            t1 = time.perf_counter()
            r = ref.filter_translations(n, s["edges"], s["orientations"], s["rel"], axes=got["axes"], rotated=got["rotated"])
            row.update(restatement_cpu_ms=round(1e3 * (time.perf_counter() - t1), 1),
                       restatement_equal=bool(np.array_equal(r["removed"], removed)),
                       restatement_min_gap=float(r["min_gap"]), restatement_threshold_margin=float(r["threshold_margin"]))
        out[f"{n}x{pairs}"] = row
        print(json.dumps({f"{n}x{pairs}": row}), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
