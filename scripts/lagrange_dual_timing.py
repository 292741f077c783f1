"""Times theia_hip_lagrange_dual_rotations at the project's two view-graph sizes (1 000 views / 40 000 pairs and 5 000
views / 250 000 pairs; tests/lagrange_dual_scenes.py's recipe: the chain plus random pairs, 2 degrees of noise, no
outliers), in both sweep orders.  The BCM is timed apart from the certificate (solver_type RANK_DEFICIENT_BCM), the
staircase with its dense certificate once per size.  Every figure is one call after one warm-up call, wall clock around
the C-ABI call; ms per sweep = the summary's sweep_ms / sweeps.  The only baseline at hand is the numpy restatement
(tests/lagrange_dual_ref.py), timed on the smaller graph for one sweep.  Prints one JSON line per measurement."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pytheiasfm_amd import global_pose as gp   # noqa: E402
from tests import lagrange_dual_scenes as sc   # noqa: E402


def main():
    for views, pairs in ((1000, 40000), (5000, 250000)):
        s = sc.make_scene(views, pairs, 2.0, 0.0, 5)
        for staircase in (False, True):
            for order in (gp.SweepOrder.INDEX, gp.SweepOrder.COLOURED):
                o = gp.SDPSolverOptions()
                o.sweep_order = order
                o.solver_type = gp.SDPSolverType.RIEMANNIAN_STAIRCASE if staircase else gp.SDPSolverType.RANK_DEFICIENT_BCM
                if staircase and order == gp.SweepOrder.INDEX:
                    continue
                for rep in range(2):
                    t0 = time.perf_counter()
                    rc, aa, est, sm = gp.lagrange_dual_rotations(s["n"], s["edges"], s["rel"], o)
                    ms = (time.perf_counter() - t0) * 1e3
                assert rc == 0
                print(json.dumps(dict(views=views, pairs=pairs, order=order.name, staircase=staircase, call_ms=round(ms, 3),
                                      sweeps=sm.sweeps, levels=sm.schedule_levels, launches_per_sweep=sm.schedule_launches,
                                      ms_per_sweep=round(sm.sweep_ms / max(sm.sweeps, 1), 4), setup_ms=round(sm.setup_ms, 3),
                                      sweep_ms=round(sm.sweep_ms, 3), certificate_ms=round(sm.certificate_ms, 3),
                                      end=gp.LAGRANGE_DUAL_END_STATES[sm.end_state], f=sm.f)), flush=True)
        if views == 1000:
            from tests import lagrange_dual_ref as ref
            Q, adj = ref.build_problem(views, s["edges"], s["rel"])
            t0 = time.perf_counter()
            ref.bcm(Q, adj, np.zeros((3, 3 * views)), ref.Options(max_iterations=1))
            print(json.dumps(dict(views=views, pairs=pairs, numpy_restatement_ms_per_sweep=round((time.perf_counter() - t0) * 1e3, 1))),
                  flush=True)


if __name__ == "__main__":
    main()
