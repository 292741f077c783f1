"""Times theia_hip_graph_match (csrc/graph_match.hip) at two sizes of a real run, global descriptors of dim 128:
1 000 images / k = 20 and 10 000 images / k = 100 (the reference's default k).  The descriptors are seeded: 50 cluster centres,
the images spread around them, the shape pooled descriptors have; the cost of the kNN search does not depend on the data, the
cost of the expansion does (through the lengths of the inverse lists).

Per size: one warm-up call, then --repeats timed calls, each the host clock around the whole C-ABI call, which uploads the
descriptors, runs every kernel and ends in the download of the pairs (a device synchronise).  The call asks with a capacity
that holds the count, so it is ONE call, pairs included.  Reported: every sample, their median, minimum and maximum.

The only baseline at hand is the single-thread Python restatement (float64 numpy distances and a stable argsort for the kNN
lists, then tests/graph_match_ref.graph_match_rows): it is timed at the first size, and at the second only with
--restatement-at-large (minutes).  Where it runs, its pairs must equal the device's on the device's own kNN lists.

Per-kernel times come from a run of their own, one size at a time, both calls (warm-up and timed) in the trace: divide by two
  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python scripts/time_graph_match.py --only 10000 100 --repeats 1 --no-restatement --out <file>
Writes profiles/graph_match.json (or --out FILE) and prints the same JSON line."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pytheiasfm_amd import _capi as capi  # noqa: E402

SIZES = [(1000, 20), (10000, 100)]


def descriptors(n, dim, seed=30, clusters=50):
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((clusters, dim))
    return (centres[rng.integers(0, clusters, size=n)] + 0.3 * rng.standard_normal((n, dim)) + 40.0).astype(np.float32)


def measure(n, k, dim, repeats, restatement):
    g = np.ascontiguousarray(descriptors(n, dim))
    P = capi.ptr
    count = C.c_int64(0)
    stats = capi.GraphMatchStats()
    capi.check(capi.lib().theia_hip_graph_match(n, dim, P(g, C.c_float), k, 0, None, None, C.byref(count), None, None, None))
    capacity = count.value
    p1 = np.zeros(capacity, np.int32); p2 = np.zeros(capacity, np.int32)
    knn_index = np.zeros((n, min(n - 1, k)), np.int32)

    def call(with_knn):
        capi.check(capi.lib().theia_hip_graph_match(n, dim, P(g, C.c_float), k, capacity, P(p1, C.c_int32), P(p2, C.c_int32),
                                                    C.byref(count), P(knn_index, C.c_int32) if with_knn else None, None,
                                                    C.byref(stats)))

    call(False)   # warm-up
    samples = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call(False)
        samples.append(1e3 * (time.perf_counter() - t0))
    row = dict(images=n, dim=dim, num_nearest_neighbors=k, all_pairs=n * (n - 1) // 2, stats=stats.as_dict(),
               selected_share=round(stats.num_pairs / (n * (n - 1) // 2), 4), call_ms_samples=[round(s, 2) for s in samples],
               call_ms_median=round(float(np.median(samples)), 2), call_ms_min=round(min(samples), 2),
               call_ms_max=round(max(samples), 2),
               timed="host clock around one whole call (upload, kernels, download of the pairs) after one warm-up call")
    if restatement:
        from tests import graph_match_ref as ref
        call(True)
        t0 = time.perf_counter()
        g64 = g.astype(np.float64)
        sq = (g64 * g64).sum(1)
        d = sq[:, None] + sq[None, :] - 2.0 * (g64 @ g64.T)
        np.fill_diagonal(d, np.inf)
        np.argsort(d, axis=1, kind="stable")[:, :k]                  # the baseline's own kNN lists: timed, not compared (other arithmetic)
        t_knn = time.perf_counter() - t0
        t0 = time.perf_counter()
        rows, _ = ref.graph_match_rows(knn_index)                    # on the device's lists, so that the pairs are comparable
        t_rows = time.perf_counter() - t0
        row["restatement_single_thread_python_s"] = dict(knn_numpy_float64=round(t_knn, 3), rows=round(t_rows, 3),
                                                         total=round(t_knn + t_rows, 3))
        row["equal_to_restatement"] = bool(np.array_equal(np.stack([p1, p2], 1), np.asarray(rows, np.int32).reshape(-1, 2)))
        row["restatement_over_call"] = round(1e3 * (t_knn + t_rows) / row["call_ms_median"], 1)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", type=int, nargs=2, metavar=("IMAGES", "K"))
    ap.add_argument("--no-restatement", action="store_true")
    ap.add_argument("--restatement-at-large", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "graph_match.json"))
    a = ap.parse_args()
    rows = []
    for n, k in ([tuple(a.only)] if a.only else SIZES):
        restatement = not a.no_restatement and (n <= 1000 or a.restatement_at_large)
        rows.append(measure(n, k, a.dim, a.repeats, restatement))
        print(json.dumps(rows[-1]), flush=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(rows, indent=1) + "\n")
    if any(not r.get("equal_to_restatement", True) for r in rows):
        sys.exit("the device result differs from the restatement")


if __name__ == "__main__":
    main()
