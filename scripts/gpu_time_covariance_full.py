"""GPU box: one theia_hip_ba_covariance_full call, all cameras and all points, after a short solve: wall time, the device
time of its phases (linearisation + Jacobians + copy, factorisation, column solves, block kernels) and the device memory
its workspace takes.  Default sizes: 200 views / 50 000 tracks and BASELINE's 1 000 views / 500 000 tracks (n = 6 000).
usage: gpu_time_covariance_full.py [views tracks]..."""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from pytheiasfm_amd import ba, synth

args = [int(a) for a in sys.argv[1:]]
sizes = list(zip(args[0::2], args[1::2])) or [(200, 50000), (1000, 500000)]
for nv, nt in sizes:
    p = synth.synth_ba_v1(nv, nt, fix_gauge=True)
    o = ba.default_options(); o.max_num_iterations = 5; o.use_inner_iterations = 0
    nobs = p.obs_uv.shape[0]
    with ba.BaHandle(p, o) as h:
        h.run()
        n = h.plan_info()["n"]
        h.covariance_full(cameras=True, points=True, view_sel=[1], track_sel=[0])     # warm-up: code objects, pools
        runs = []
        for _ in range(3):
            t0 = time.perf_counter()
            cc, pc = h.covariance_full(cameras=True, points=True)
            runs.append((time.perf_counter() - t0, h.covariance_full_timing()))
        wall, ph = min(runs, key=lambda r: r[0])
        chunk = min(n, 1024)
        work = 8 * ((n + 1) * (n + 1) + n * n + 2 * chunk * n + 18 * nobs + 9 * nt + 36 * nv) + 8 * nt
        print(json.dumps({"views": nv, "tracks": nt, "observations": int(nobs), "n": n, "wall_ms": round(1e3 * wall, 2),
                          "linearise_ms": round(ph["linearise"], 2), "factor_ms": round(ph["factor"], 2),
                          "solve_ms": round(ph["solve"], 2), "blocks_ms": round(ph["blocks"], 2),
                          "workspace_mb": round(work / 1e6, 1), "X_mb": round(8 * n * n / 1e6, 1),
                          "walls_ms": [round(1e3 * r[0], 2) for r in runs],
                          "cameras_done": int(np.count_nonzero(cc.reshape(nv, -1)[:, 0])),
                          "points_done": int(np.count_nonzero(pc.reshape(nt, -1)[:, 0]))}), flush=True)
