"""Times the co-visibility entries (csrc/covisibility.hip) on two reconstructions whose tracks run along a camera path:
1 000 views x 5 000 observations per view and 5 000 views x 5 000.  A track is seen by 3 .. 40 consecutive views of the
path, so a view shares tracks with the 39 views on either side of it; the points lie beside the path.  Per case: WARMUP
calls, then REPEAT timed calls of each whole entry point (host clock; a call covers the checks, the host plan, the upload,
the launches and the download): median, smallest, largest and the quartiles, in milliseconds -- the graph with its edge
data (min_shared_tracks 10), the scores of its pairs, the whole view selection (10 neighbours), and 10 000 common-track
queries of 2 .. 6 neighbouring views.  Also the number of edges, the degrees, and a digest of the outputs, which two builds
of the library must share.  At 1 000 views the sequential restatement (tests/covisibility_ref.py) is timed on a sample of
view pairs and scaled to all pairs, for scale only: it says nothing about the reference's C++.
Per-launch times come from a run of their own:
  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python scripts/gpu_time_covisibility.py 1000
Another build of the library is named by THEIA_HIP_LIBRARY.  Arguments: the view counts to run (default: both); run each size
as a command of its own under `timeout -k 10 <seconds>` (240 s and 420 s are ample).  Prints one JSON line."""
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pytheiasfm_amd import _capi as capi, covisibility as cv  # noqa: E402
from tests import covisibility_ref as ref  # noqa: E402

WARMUP, REPEAT = 2, 10
OBS_PER_VIEW, MIN_LEN, MAX_LEN = 5000, 3, 40
THETA0, SIGMA1, SIGMA2 = 5.0, 1.0, 10.0
RESTATEMENT_PAIRS = 400


def path_scene(num_views, seed=1):
    rng = np.random.default_rng(seed)
    mean_len = 0.5 * (MIN_LEN + MAX_LEN)
    num_tracks = int(num_views * OBS_PER_VIEW / mean_len)
    length = rng.integers(MIN_LEN, MAX_LEN + 1, num_tracks)
    first = rng.integers(0, num_views, num_tracks)
    obs_track = np.repeat(np.arange(num_tracks, dtype=np.int32), length)
    within = np.arange(len(obs_track)) - np.repeat(np.cumsum(length) - length, length)
    obs_view = ((np.repeat(first, length) + within) % num_views).astype(np.int32)
    order = rng.permutation(len(obs_view))
    s = np.arange(num_views, dtype=np.float64)
    cam_ext = np.zeros((num_views, 6))
    cam_ext[:, 0] = s; cam_ext[:, 1] = 3.0 * np.sin(0.05 * s); cam_ext[:, 2] = rng.uniform(-0.5, 0.5, num_views)
    cam_ext[:, 3:6] = rng.standard_normal((num_views, 3)) * 0.3
    mid = (first + 0.5 * length) % num_views
    points = np.stack([mid + rng.uniform(-5, 5, num_tracks), rng.uniform(15, 40, num_tracks), rng.uniform(-5, 5, num_tracks),
                       np.ones(num_tracks)], axis=1)
    return dict(num_views=num_views, num_tracks=num_tracks, obs_view=np.ascontiguousarray(obs_view[order]),
                obs_track=np.ascontiguousarray(obs_track[order]), cam_ext=cam_ext, points=points)


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
    out = dict(library=os.path.basename(capi.LIB_PATH), warmup=WARMUP, repeat=REPEAT, obs_per_view=OBS_PER_VIEW)
    sizes = [int(a) for a in sys.argv[1:]] or [1000, 5000]
    for n in sizes:
        s = path_scene(n)
        a = (s["num_views"], s["num_tracks"], s["obs_view"], s["obs_track"])
        (pairs, shared, rot, pos), graph = timed(lambda: cv.covisibility_graph(*a, None, None, s["cam_ext"], 10))
        (_, _, _, _), counts_only = timed(lambda: cv.covisibility_graph(*a, None, None, None, 10))
        (score, common), scores = timed(lambda: cv.mvsnet_pair_scores(*a, s["cam_ext"], s["points"], pairs, THETA0, SIGMA1, SIGMA2))
        (neighbor, nscore), selection = timed(lambda: cv.view_selection_mvsnet(*a, None, None, s["cam_ext"], s["points"], 10,
                                                                              THETA0, SIGMA1, SIGMA2))
        rng = np.random.default_rng(2)
        queries = [((int(f) + np.arange(int(k))) % n).tolist() for f, k in zip(rng.integers(0, n, 10000), rng.integers(2, 7, 10000))]
        answers, common_tracks = timed(lambda: cv.find_common_tracks(*a, queries))
        degree = np.bincount(pairs.reshape(-1), minlength=n)
        digest = hashlib.sha256(pairs.tobytes() + shared.tobytes() + rot.tobytes() + pos.tobytes() + score.tobytes()
                                + common.tobytes() + neighbor.tobytes() + nscore.tobytes() + np.concatenate(answers).tobytes())
        row = dict(observations=len(s["obs_view"]), tracks=s["num_tracks"], edges=len(pairs), degree_min=int(degree.min()),
                   degree_max=int(degree.max()), shared_max=int(shared.max()), common_tracks_found=int(sum(len(x) for x in answers)),
                   graph_with_edge_data=graph, graph_pairs_only=counts_only, pair_scores=scores, view_selection=selection,
                   find_common_tracks_10000_queries=common_tracks, digest=digest.hexdigest()[:16])
        if n == 1000:
            lists = ref.tracks_by_view(n, s["obs_view"], s["obs_track"])
            sample = np.random.default_rng(3).integers(0, n, (RESTATEMENT_PAIRS, 2))
            t0 = time.perf_counter()
            for i, j in sample.tolist():
                ref.intersect(lists[i], lists[j])
            per_pair = (time.perf_counter() - t0) / RESTATEMENT_PAIRS
            row.update(restatement_sampled_pairs=RESTATEMENT_PAIRS, restatement_ms_per_pair=round(1e3 * per_pair, 3),
                       restatement_all_pairs_seconds_scaled=round(per_pair * n * (n - 1) / 2, 1))
        out[f"{n}x{OBS_PER_VIEW}"] = row
        print(json.dumps({f"{n}x{OBS_PER_VIEW}": row}), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
