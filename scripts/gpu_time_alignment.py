"""Times the reconstruction-alignment entry points (csrc/alignment.hip) at the sizes the section quotes:
    umeyama_batch      theia_hip_align_point_clouds, 1 000 problems x 1 000 points
    umeyama_single     one problem of 1 000 000 points
    transform          theia_hip_transform_reconstruction, 1 000 cameras + 500 000 points
    robust             THEIA_EST_CAMERA_ALIGNMENT, 1 000 problems x 200 cameras x 1 000 iterations (min = max), use_mle
    align_rotations    theia_hip_align_rotations, 5 000 rotations, planted alignment of 1 rad, noise 1e-3
Per row: WARMUP calls, then REPEAT timed calls; median, smallest and largest of the call (host clock over the whole entry:
checks, upload, kernels, download) and, where the entry reports it, of the kernels alone (device events).  The Umeyama rows
also time the numpy restatement of tests/alignment_ref.py on the same input (one pass, no device) -- the only baseline at
hand.  The transform row quotes the bytes the kernel moves over 6.3 TB/s, the rate a streaming copy reaches on the MI355X's
HBM.  Prints one JSON line."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pytheiasfm_amd import alignment, ransac, sfm  # noqa: E402
from tests import alignment_ref as ar  # noqa: E402
from tests import alignment_scenes as sc  # noqa: E402

WARMUP, REPEAT = 1, 5
HBM_BYTES_PER_S = 6.3e12


def spread(ms):
    return dict(median_ms=round(float(np.median(ms)), 4), min_ms=round(float(np.min(ms)), 4), max_ms=round(float(np.max(ms)), 4))


def timed(call, with_kernel=True):
    for _ in range(WARMUP):
        call([])
    wall, kern = [], []
    for _ in range(REPEAT):
        tm = []
        t0 = time.perf_counter()
        out = call(tm)
        wall.append(1e3 * (time.perf_counter() - t0))
        if tm:
            kern.append(tm[0])
    d = dict(call=spread(wall))
    if with_kernel and kern:
        d["kernel"] = spread(kern)
    return out, d


def clouds(num, n, rng):
    lefts, rights = [], []
    for _ in range(num):
        R, t, s = sc.planted_similarity(rng)
        left = rng.uniform(-5, 5, (n, 3))
        lefts.append(left); rights.append(s * left @ R.T + t + rng.uniform(-1e-3, 1e-3, (n, 3)))
    return lefts, rights


def umeyama(num, n, rng):
    lefts, rights = clouds(num, n, rng)
    (R, t, s, st), d = timed(lambda tm: alignment.align_point_clouds_batch(lefts, rights, timings=tm))
    t0 = time.perf_counter()
    ref = [ar.umeyama(a, b) for a, b in zip(lefts, rights)]
    d["numpy_restatement_ms"] = round(1e3 * (time.perf_counter() - t0), 2)
    d["max_deviation"] = float(max(max(np.abs(R[p] - u["R"]).max(), abs(s[p] / u["s"] - 1.0)) for p, u in enumerate(ref)))
    d["degenerate"] = int(st.sum())
    return d


def transform(nc, npt, rng):
    r = sfm.Reconstruction()
    r.cam_ext = np.hstack([rng.uniform(-5, 5, (nc, 3)), rng.uniform(-1, 1, (nc, 3))])
    r.view_estimated = np.ones(nc, dtype=bool)
    r.points = np.hstack([rng.uniform(-5, 5, (npt, 3)), np.ones((npt, 1))])
    r.track_estimated = np.ones(npt, dtype=bool)
    R, t, s = sc.planted_similarity(rng)
    _, d = timed(lambda tm: alignment.TransformReconstruction(r, R, t, 1.0, timings=tm))
    moved = 2 * (48 * nc + 32 * npt) + nc + npt     # every row read and written once, and its mask byte
    d["bytes_moved"] = moved
    d["floor_ms"] = round(1e3 * moved / HBM_BYTES_PER_S, 5)
    d["kernel_over_floor"] = round(d["kernel"]["median_ms"] / (1e3 * moved / HBM_BYTES_PER_S), 1)
    return d


def robust(num, n, iters, rng):
    rows = [sc.camera_problem(rng, n=n, num_outliers=n // 4)[0] for _ in range(num)]
    p = ransac.RansacParameters()
    p.error_thresh = 0.05 ** 2; p.min_iterations = iters; p.max_iterations = iters; p.use_mle = True; p.seed = 1
    data = np.concatenate(rows)
    offsets = np.arange(num + 1, dtype=np.int64) * n
    res, d = timed(lambda tm: ransac.estimate_batch(ransac.EST_CAMERA_ALIGNMENT, data, offsets, p), with_kernel=False)
    d["hypotheses"] = int(res["hypotheses_evaluated"])
    d["hypotheses_per_s_call"] = round(res["hypotheses_evaluated"] / (1e-3 * d["call"]["median_ms"]))
    d["hypotheses_per_s_fit_score"] = round(res["hypotheses_evaluated"] / res["time_fit_score_seconds"])
    d["successes"] = int(res["success"].sum())
    return d


def rotations(n):
    gt, rot, _ = sc.align_rotations_scene(n, "one_radian")
    (_, w, summ, _), d = timed(lambda tm: alignment.align_rotations(gt, rot), with_kernel=False)
    d.update(iterations=int(summ.iterations), termination=int(summ.termination), final_cost=float(summ.final_cost))
    return d


def main():
    rng = np.random.default_rng(0)
    out = dict(warmup=WARMUP, repeat=REPEAT)
    for name, run in (("umeyama_batch_1000x1000", lambda: umeyama(1000, 1000, rng)),
                      ("umeyama_single_1000000", lambda: umeyama(1, 1000000, rng)),
                      ("transform_1000_cameras_500000_points", lambda: transform(1000, 500000, rng)),
                      ("robust_1000x200x1000", lambda: robust(1000, 200, 1000, rng)),
                      ("align_rotations_5000", lambda: rotations(5000))):
        out[name] = run()
        print(json.dumps({name: out[name]}), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
