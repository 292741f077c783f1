"""Times theia_hip_optimize_alignment_sim3 on the GPU: 1 000 problems x 1 000 points on the group route, one
problem of 500 000 points on each route, and one problem of n points on each route for the n around
THEIA_SIM3_GROUP_MAX_POINTS (the threshold was picked from these).  Every figure is ONE timed call after one untimed call
of the same shape; kernel ms are device events around the call's kernels, call ms the whole C entry.
    python scripts/gpu_time_sim3_alignment.py"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytheiasfm_amd import alignment as al  # noqa: E402
from tests import sim3_ref as ref          # noqa: E402

GT = ref.create_sim3([1.0, 2.0, 0.5], [0.1, 0.05, 0.02], 1.5)
START = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0])


def clouds(count, n, rng):
    src = [ref.synthetic_cloud(n, 0.01, rng) for _ in range(count)]
    return src, [ref.transform_cloud(s, GT) + rng.normal(0.0, 0.01, size=s.shape) for s in src]


def timed(src, tgt, group_max=None):
    if group_max is None:
        os.environ.pop("THEIA_HIP_SIM3_GROUP_MAX_POINTS", None)
    else:
        os.environ["THEIA_HIP_SIM3_GROUP_MAX_POINTS"] = str(group_max)
    opts = [al.Sim3AlignmentOptions() for _ in src]
    starts = [START] * len(src)
    al.optimize_alignment_sim3(src, tgt, starts, opts)
    tm = [0.0, 0.0]
    _, summ, _ = al.optimize_alignment_sim3(src, tgt, starts, opts, timings=tm)
    return dict(kernel_ms=round(tm[0], 4), call_ms=round(tm[1], 4), route=summ[0].route, iterations=summ[0].num_iterations,
                success=summ[0].success)


def main():
    rng = np.random.default_rng(7)
    out = {}
    s, t = clouds(1000, 1000, rng)
    out["1000x1000 group"] = timed(s, t)
    s, t = clouds(1, 500000, rng)
    out["1x500000 group"] = timed(s, t, 10 ** 9)
    out["1x500000 grid"] = timed(s, t, 1)
    for n in (2048, 4096, 8192, 16384, 32768, 65536):
        s, t = clouds(1, n, rng)
        out[f"1x{n} group"] = timed(s, t, 10 ** 9)
        out[f"1x{n} grid"] = timed(s, t, 1)
    for k, v in out.items():
        print(k, json.dumps(v))


if __name__ == "__main__":
    main()
