"""Times theia_hip_brute_force_match_pairs (csrc/brute_force_matcher.hip) at the size of a real SfM run: 64 images of 5 000
features, descriptors of dim 128, 500 image pairs (the first 500 of all pairs i < j), default options.  The descriptors are
seeded unit-norm random vectors: the cost of the matcher does not depend on the data.  One warm-up call, then one timed call:
the host clock around the whole C-ABI call, which uploads the descriptors, runs every chunk of pairs and ends in the download
of the last chunk's matches (a device synchronise).  The multiply-add rate counts the 2 n1 n2 dim operations of each pair's
distance matrix -- ONE matrix per pair, where the reference computes two -- over that whole-call time, so it is an end-to-end
figure, below the tile kernel's own rate; it is given as a fraction of the 157.3 TF FP32 matrix peak and of the 122 TF an
untuned LDS-tiled FP32-MFMA GEMM reaches.  Per-kernel times come from a run of their own:
  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python scripts/time_brute_force_matcher.py
Writes profiles/bf_matcher.json (or --out FILE) and prints the same JSON line."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pytheiasfm_amd import _capi as capi, matching  # noqa: E402

PEAK_TF, UNTUNED_GEMM_TF = 157.3, 122.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--features", type=int, default=5000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--pairs", type=int, default=500)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bf_matcher.json"))
    a = ap.parse_args()
    rng = np.random.default_rng(20)
    descs = []
    for _ in range(a.images):
        d = rng.standard_normal((a.features, a.dim)).astype(np.float32)
        descs.append(d / np.linalg.norm(d, axis=1, keepdims=True))
    pairs = [(i, j) for i in range(a.images) for j in range(i + 1, a.images)][:a.pairs]
    o = matching.FeatureMatcherOptions().to_c()
    flat = np.ascontiguousarray(np.concatenate(descs))
    feat_off = (a.features * np.arange(a.images + 1)).astype(np.int64)
    p1 = np.array([p[0] for p in pairs], np.int32); p2 = np.array([p[1] for p in pairs], np.int32)
    cap = a.features * len(pairs)
    ok = np.zeros(len(pairs), np.uint8); off = np.zeros(len(pairs) + 1, np.int64)
    f1 = np.zeros(cap, np.int32); f2 = np.zeros(cap, np.int32); dist = np.zeros(cap, np.float32)
    P = capi.ptr

    def call():
        capi.check(capi.lib().theia_hip_brute_force_match_pairs(
            a.images, P(feat_off, C.c_int64), a.dim, P(flat, C.c_float), len(pairs), P(p1, C.c_int32), P(p2, C.c_int32), C.byref(o),
            P(ok, C.c_uint8), P(off, C.c_int64), P(f1, C.c_int32), P(f2, C.c_int32), P(dist, C.c_float)))

    call()   # warm-up
    t0 = time.perf_counter()
    call()
    seconds = time.perf_counter() - t0
    flop = 2.0 * a.features * a.features * a.dim * len(pairs)
    tf = flop / seconds / 1e12
    row = dict(images=a.images, features_per_image=a.features, dim=a.dim, pairs=len(pairs), call_ms=round(1e3 * seconds, 2),
               pairs_per_second=round(len(pairs) / seconds, 1), fp32_multiply_add_tflops=round(tf, 2),
               fraction_of_matrix_peak_157tf=round(tf / PEAK_TF, 4), fraction_of_untuned_mfma_gemm_122tf=round(tf / UNTUNED_GEMM_TF, 4),
               pairs_ok=int(ok.sum()), matches=int(off[-1]), timed="host clock around one whole call after one warm-up call")
    with open(a.out, "w") as f:
        f.write(json.dumps(row, indent=1) + "\n")
    print(json.dumps(row))


if __name__ == "__main__":
    main()
