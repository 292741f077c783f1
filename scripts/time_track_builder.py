"""Times theia_hip_build_tracks (csrc/track_builder.hip) at the size of a 1 000-view reconstruction: 1 000 views of 5 000 features,
20 000 image pairs of 300 matches each (6 M correspondences), min 2 / max 50.

The scene: 200 000 points on a ring, view v sees the 5 000 points from 200 v on, each at a feature index of its own (a seeded
permutation per view), so a point is seen by 25 consecutive views; the pairs are (v, v + d) for d = 1 .. 20; a pair's matches are
300 of the points the two views share, drawn with a seed, and every second pair adds one random match (an outlier that joins two
tracks: some components pass the cap and go through the host replay).

The GPU step runs in a child process of its own under `timeout -k 10`: one warm-up call, then ONE timed call -- the host clock
around the whole C-ABI call, and the library's own split of it (theia_hip_track_builder_last_timings: upload, components, replay
on the host, emit, download; each phase ends in a device synchronise).  The parent then times, on the same scene and the same
machine, the single-thread restatement tests/track_builder_ref.py -- the only baseline there is without the reference's C++
TrackBuilder -- and checks that the two results are equal.  Writes profiles/track_builder.json (or --out FILE) and prints the
same JSON line."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEP = 200        # a view's window of points starts STEP points after its predecessor's


def scene(views, features, neighbours, matches, seed=21):
    rng = np.random.default_rng(seed)
    feature_of = np.stack([rng.permutation(features) for _ in range(views)]).astype(np.int32)   # [view][local point]
    pv1 = np.repeat(np.arange(views), neighbours).astype(np.int32)
    gap = np.tile(np.arange(1, neighbours + 1), views)
    pv2 = ((pv1 + gap) % views).astype(np.int32)
    counts = np.full(len(pv1), matches, np.int64)
    counts[1::2] += 1
    match_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    f1 = np.empty(match_off[-1], np.int32); f2 = np.empty(match_off[-1], np.int32)
    for k in range(len(pv1)):
        shared = features - gap[k] * STEP                 # local points 0 .. shared - 1 of view 2 are gap * STEP .. of view 1
        pick = rng.choice(shared, matches, replace=False)
        a = match_off[k]
        f1[a:a + matches] = feature_of[pv1[k], pick + gap[k] * STEP]
        f2[a:a + matches] = feature_of[pv2[k], pick]
        if counts[k] > matches:
            f1[a + matches] = rng.integers(features); f2[a + matches] = rng.integers(features)
    feat_off = features * np.arange(views + 1, dtype=np.int64)
    return feat_off, pv1, pv2, match_off, f1, f2


def gpu_step(scene_file, out_file, max_len):
    from pytheiasfm_amd import tracks
    with np.load(scene_file) as z:
        graph = tuple(z[k] for k in ("feat_off", "pv1", "pv2", "match_off", "f1", "f2"))
    opt = tracks.TrackBuilderOptions(2, max_len)
    tracks.build_tracks(*graph, opt)     # warm-up
    t0 = time.perf_counter()
    track_off, obs_view, obs_feature, obs_track, stats = tracks.build_tracks(*graph, opt)
    seconds = time.perf_counter() - t0
    split = tracks.last_timings()
    np.savez(out_file, track_off=track_off, obs_view=obs_view, obs_feature=obs_feature, obs_track=obs_track,
             meta=json.dumps(dict(call_ms=round(1e3 * seconds, 2), split_ms={k: round(v, 2) for k, v in split.items()}, stats=stats)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=1000)
    ap.add_argument("--features", type=int, default=5000)
    ap.add_argument("--neighbours", type=int, default=20)
    ap.add_argument("--matches", type=int, default=300)
    ap.add_argument("--max-track-length", type=int, default=50)
    ap.add_argument("--gpu-timeout", type=int, default=240)
    ap.add_argument("--no-restatement", action="store_true", help="skip the single-thread baseline (and the equality check)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_builder.json"))
    ap.add_argument("--gpu-step", nargs=2, metavar=("SCENE", "RESULT"), help="(internal) the child process")
    a = ap.parse_args()
    if a.gpu_step:
        gpu_step(a.gpu_step[0], a.gpu_step[1], a.max_track_length)
        return
    graph = scene(a.views, a.features, a.neighbours, a.matches)
    print(f"scene: {a.views} views, {len(graph[1])} pairs, {int(graph[3][-1])} correspondences", flush=True)
    with tempfile.TemporaryDirectory() as tmp:
        scene_file, result_file = os.path.join(tmp, "scene.npz"), os.path.join(tmp, "result.npz")
        np.savez(scene_file, **dict(zip(("feat_off", "pv1", "pv2", "match_off", "f1", "f2"), graph)))
        subprocess.check_call(["timeout", "-k", "10", str(a.gpu_timeout), sys.executable, os.path.abspath(__file__), "--gpu-step",
                               scene_file, result_file, "--max-track-length", str(a.max_track_length)])
        with np.load(result_file) as z:
            got = [z[k] for k in ("track_off", "obs_view", "obs_feature", "obs_track")]
            meta = json.loads(str(z["meta"]))
    stats = meta["stats"]
    m = int(graph[3][-1])
    row = dict(views=a.views, features_per_view=a.features, pairs=len(graph[1]), correspondences=m, min_track_length=2,
               max_track_length=a.max_track_length, call_ms=meta["call_ms"], split_ms=meta["split_ms"],
               correspondences_per_second=round(m / (1e-3 * meta["call_ms"])), stats=stats,
               replayed_share_of_correspondences=round(stats["num_replayed_correspondences"] / m, 6),
               timed="host clock around one whole call after one warm-up call; split by the library's own phase clocks")
    print(json.dumps(row), flush=True)
    if not a.no_restatement:
        from tests import track_builder_ref as ref
        t0 = time.perf_counter()
        want = ref.build_tracks(*graph, 2, a.max_track_length)
        row["restatement_single_thread_python_s"] = round(time.perf_counter() - t0, 2)
        row["equal_to_restatement"] = bool(all(np.array_equal(g, w) for g, w in zip(got, want[:4])) and stats == want[4])
        row["restatement_over_call"] = round(1e3 * row["restatement_single_thread_python_s"] / meta["call_ms"], 1)
    with open(a.out, "w") as f:
        f.write(json.dumps(row, indent=1) + "\n")
    print(json.dumps(row))
    if not row.get("equal_to_restatement", True):
        sys.exit("the device result differs from the restatement")


if __name__ == "__main__":
    main()
