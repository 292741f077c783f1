"""GPU box: the streams entry point (theia_hip_ransac_estimate_streams) against the seeded one on five-point relative pose with
adaptive termination, 1000 pairs x 2000 correspondences: problems/s and hypotheses/s for 1, 8, 64 and 1000 streams (the
pairs dealt round-robin), and the same pairs through theia_hip_ransac_estimate_batch.
usage: gpu_time_ransac_streams.py [pairs] [repeats]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytheiasfm_amd import ransac, synth  # noqa: E402

NP = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
REP = int(sys.argv[2]) if len(sys.argv) > 2 else 3
data, offsets, _ = synth.synth_ransac_v1(NP, 2000, "relative", seed=0x5AC50005)
p = ransac.RansacParameters(); p.error_thresh = (2.0 / 1000.0) ** 2; p.min_iterations = 100; p.max_iterations = 5000
p.failure_probability = 1e-3; p.seed = 1
pc = p.to_c()
ransac.estimate_batch(0, data[:offsets[8]], offsets[:9], pc)   # warm-up: device, pools, kernels


def best(fn):
    times, res = [], None
    for _ in range(REP):
        t0 = time.perf_counter(); res = fn(); times.append(time.perf_counter() - t0)
    return min(times), float(np.median(times)), res


t, tm, res = best(lambda: ransac.estimate_batch(0, data, offsets, pc))
h = res["hypotheses_evaluated"]
print(f"seeded      : {NP / t:9.1f} problems/s  {h / t / 1e6:7.2f} M hyp/s  (best {t * 1e3:.1f} ms, median {tm * 1e3:.1f} ms, {h} hypotheses)", flush=True)
for ns in (1000, 64, 8, 1):
    if ns > NP:
        continue
    sop = np.arange(NP) % ns

    def run():
        st = ransac.rng_states(ns, [1 + k for k in range(ns)])
        return ransac.estimate_batch(0, data, offsets, pc, streams=(st, sop))
    t, tm, res = best(run)
    h = res["hypotheses_evaluated"]
    print(f"{ns:4d} streams : {NP / t:9.1f} problems/s  {h / t / 1e6:7.2f} M hyp/s  (best {t * 1e3:.1f} ms, median {tm * 1e3:.1f} ms, {h} hypotheses)", flush=True)
