"""Times theia_hip_visibility_scores and theia_hip_set_underconstrained_unestimated (csrc/next_view.hip) at 1 000 views x
5 000 observations and 5 000 x 5 000: six pyramid levels, half the tracks estimated, every observation of a view on a track
of its own, 1920 x 1080 images, coordinates uniform over the image.  Per size: WARMUP calls, then REPEAT timed calls of the
whole entry point (host clock; the call ends in the copy of its results back, so it covers the checks, the upload, the
launches and the download): median, smallest, largest and the quartiles, in milliseconds, with a digest of the outputs.
`restatement` as an argument times the plain-loop restatements of tests/incremental_ref.py on the smaller size instead (one
call each, no device), and prints their digests, which equal the device's.  Prints one JSON line."""
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pytheiasfm_amd import incremental as inc  # noqa: E402
from tests import incremental_ref as ref  # noqa: E402

WARMUP, REPEAT = 2, 10
SIZE = (1920, 1080)


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


def scene(num_views, per_view, seed=1):
    rng = np.random.default_rng(seed)
    num_tracks = 40 * num_views * per_view // 1000     # a track is seen by 25 views on average
    obs_track = np.concatenate([rng.choice(num_tracks, size=per_view, replace=False) for _ in range(num_views)]).astype(np.int32)
    obs_view = np.repeat(np.arange(num_views, dtype=np.int32), per_view)
    off = np.arange(num_views + 1, dtype=np.int64) * per_view
    uv = rng.uniform(0.0, 1.0, size=(len(obs_track), 2)) * np.array(SIZE, dtype=np.float64)
    track_estimated = (rng.random(num_tracks) < 0.5).astype(np.uint8)
    view_estimated = (rng.random(num_views) < 0.9).astype(np.uint8)
    return dict(nv=num_views, nt=num_tracks, off=off, uv=uv, obs_view=obs_view, obs_track=obs_track,
                track_estimated=track_estimated, view_estimated=view_estimated,
                size=np.tile(np.array(SIZE, np.int32), (num_views, 1)))


def digest(*arrays):
    return hashlib.sha256(b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)).hexdigest()[:16]


def device(s):
    (n, score), vis = timed(lambda: inc.visibility_scores(s["off"], s["uv"], s["obs_track"], s["track_estimated"], s["size"], 6))

    def sweep():
        ve, te = s["view_estimated"].copy(), s["track_estimated"].copy()
        return inc.set_underconstrained_unestimated(s["nv"], s["nt"], s["obs_view"], s["obs_track"], ve, te), ve, te
    (counts, ve, te), sw = timed(sweep)
    return dict(visibility_scores=vis, visibility_digest=digest(n.astype(np.int32), score.astype(np.int32)),
                sweep=sw, sweep_counts=list(counts), sweep_digest=digest(ve, te))


def restatement(s):
    obs_track, uv, est = s["obs_track"].tolist(), s["uv"].tolist(), s["track_estimated"].tolist()
    t0 = time.perf_counter()
    n, score = [], []
    for v in range(s["nv"]):
        p = ref.VisibilityPyramid(SIZE[0], SIZE[1], 6)
        k = 0
        for row in range(int(s["off"][v]), int(s["off"][v + 1])):
            if est[obs_track[row]]:
                k += 1
                p.add_point(uv[row][0], uv[row][1])
        n.append(k); score.append(p.compute_score())
    vis_ms = 1e3 * (time.perf_counter() - t0)
    ve, te = s["view_estimated"].astype(bool).tolist(), s["track_estimated"].astype(bool).tolist()
    obs_view = s["obs_view"].tolist()
    t0 = time.perf_counter()
    counts = ref.set_underconstrained_as_unestimated(obs_view, obs_track, ve, te)
    sweep_ms = 1e3 * (time.perf_counter() - t0)
    return dict(restatement_visibility_ms=round(vis_ms, 1), restatement_sweep_ms=round(sweep_ms, 1),
                visibility_digest=digest(np.array(n, np.int32), np.array(score, np.int32)), sweep_counts=list(counts),
                sweep_digest=digest(np.array(ve, np.uint8), np.array(te, np.uint8)))


def main():
    out = dict(warmup=WARMUP, repeat=REPEAT)
    if "restatement" in sys.argv[1:]:
        out["1000x5000"] = restatement(scene(1000, 5000))
    else:
        for nv, per_view in ((1000, 5000), (5000, 5000)):
            out[f"{nv}x{per_view}"] = device(scene(nv, per_view))
            print(json.dumps({f"{nv}x{per_view}": out[f"{nv}x{per_view}"]}), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
