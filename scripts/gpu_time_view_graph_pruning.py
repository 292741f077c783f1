"""Times theia_hip_filter_view_graph_cycles_by_rotation (csrc/view_graph_pruning.hip) and, beside it, the host-side
theia_hip_remove_disconnected_view_pairs on the two graphs the other global stages are timed on: 1 000 views / 40 000
pairs and 5 000 views / 250 000 pairs, 2 degrees of noise, 10 % outlier rotations (tests/rotation_scenes.py), threshold
4 degrees.  Per graph: WARMUP calls, then REPEAT timed calls of the whole entry point (host clock; the call ends in the
copy of its results back, so it covers the checks, the adjacency, the upload, both launches and the download): median,
smallest, largest and the quartiles, in milliseconds.  Also the triangles of the graph, the pairs removed among outliers
and inliers, and a digest of the outputs, which two builds of the library must share.  At 1 000 views the numpy restatement
(tests/view_graph_pruning_ref.py) runs too: its wall time, whether its verdicts and counts equal the device's, and the
largest difference of the finite per-pair minima.  Per-launch times come from a run of their own:
  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python scripts/gpu_time_view_graph_pruning.py
The variant with 64 lanes per pair is the same library built with -DTHEIA_CYCLE_TEAM=64 and named by THEIA_HIP_LIBRARY.
Prints one JSON line."""
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pytheiasfm_amd import _capi as capi, global_pose  # noqa: E402
from tests import rotation_scenes as rs  # noqa: E402
from tests import view_graph_pruning_ref as ref  # noqa: E402

WARMUP, REPEAT = 3, 20
WANT = ("min_loop_error_degrees", "triangles_per_pair", "num_triangles")


def spread(ms):
    q = np.percentile(ms, [0, 25, 50, 75, 100])
    return dict(median_ms=round(float(q[2]), 3), min_ms=round(float(q[0]), 3), q1_ms=round(float(q[1]), 3),
                q3_ms=round(float(q[3]), 3), max_ms=round(float(q[4]), 3))


def timed(call):
    for _ in range(WARMUP):
        call()
    ms = []
    for _ in range(REPEAT):
        t0 = time.perf_counter()
        out = call()
        ms.append(1e3 * (time.perf_counter() - t0))
    return out, spread(ms)


def main():
    out = dict(library=os.path.basename(capi.LIB_PATH), warmup=WARMUP, repeat=REPEAT)
    sizes = ((1000, 40000), (5000, 250000))
    if len(sys.argv) > 1:
        sizes = tuple(s for s in sizes if str(s[0]) in sys.argv[1:])
    for n, pairs in sizes:
        s = rs.make_scene(n, pairs, 2.0, 0.1, seed=1)
        (rc, removed, got), cycle = timed(lambda: global_pose.filter_cycles_by_rotation(n, s["edges"], s["rel"], 4.0, want=WANT))
        digest = hashlib.sha256(removed.tobytes() + got["min_loop_error_degrees"].tobytes() + got["triangles_per_pair"].tobytes())
        row = dict(rc=rc, cycle_filter=cycle, triangles=got["num_triangles"], removed=int(removed.sum()),
                   outliers=int(s["outliers"].sum()), outliers_removed=int((removed & s["outliers"]).sum()),
                   inliers_removed=int((removed & ~s["outliers"]).sum()), digest=digest.hexdigest()[:16])
        kept = np.ascontiguousarray(s["edges"][~removed])
        (rc2, gone_pairs, gone_views, _), comp = timed(lambda: global_pose.remove_disconnected_pairs(n, kept))
        row.update(rc_components=rc2, remove_disconnected=comp, pairs_after_filter=len(kept),
                   disconnected_pairs=int(gone_pairs.sum()), disconnected_views=int(gone_views.sum()))
        if n == 1000:
            t0 = time.perf_counter()
            r = ref.cycle_filter(n, s["edges"], s["rel"], 4.0)
            fin = np.isfinite(r["min_loop_error_degrees"])
            row.update(restatement_cpu_ms=round(1e3 * (time.perf_counter() - t0), 1),
                       restatement_equal=bool(np.array_equal(r["removed"], removed) and r["num_triangles"] == got["num_triangles"]
                                              and np.array_equal(r["triangles_per_pair"], got["triangles_per_pair"])
                                              and np.array_equal(fin, np.isfinite(got["min_loop_error_degrees"]))),
                       restatement_threshold_margin=float(np.abs(r["min_loop_error_degrees"][fin] - 4.0).min()),
                       largest_minimum_difference=float(np.abs(r["min_loop_error_degrees"][fin] - got["min_loop_error_degrees"][fin]).max()))
        out[f"{n}x{pairs}"] = row
        print(json.dumps({f"{n}x{pairs}": row}), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
