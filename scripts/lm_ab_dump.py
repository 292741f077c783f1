"""lm_ab_dump.py OUT.npz -- everything the Levenberg-Marquardt loops of the library hand back, for comparing two builds of
it byte for byte (a refactor of the step rules must not move a bit):

    THEIA_HIP_LIBRARY=/path/to/parent/libtheia_hip.so python scripts/lm_ab_dump.py parent.npz
    python scripts/lm_ab_dump.py branch.npz
    python scripts/lm_ab_dump.py --compare parent.npz branch.npz

Runs tests.test_lm_rules_gpu.device(case, rule, ...) for every entry of lm_rule_cases.CASE_RULES at both sides of its
bracket (every loop of the BA family, stopping by each tolerance rule), and one scene each of the nonlinear rotation and
position estimators (graph_lm.h's k_decide), and stores every returned field: termination, counts, costs, parameters, trace
arrays.  The brackets come from the CPU oracle, which is the same for both builds.  One process per library.

The inverse-depth solve (ba_invdepth.hip) sums its reduced system with floating-point atomics and is not reproducible from
run to run (1 ulp in the costs, measured); dump the parent twice, and read a difference between the builds against the
difference between the parent's two dumps: on an MI355X the same 88 of 2063 arrays, all invdepth-*, differ in either pair."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def compare(a_path, b_path):
    a, b = np.load(a_path), np.load(b_path)
    bad = sorted(set(a.files) ^ set(b.files))
    for k in sorted(set(a.files) & set(b.files)):
        x, y = a[k], b[k]
        if x.shape != y.shape or x.dtype != y.dtype or x.tobytes() != y.tobytes():
            bad.append(k)
    print(f"{len(a.files)} / {len(b.files)} arrays, {len(bad)} differ")
    for k in bad[:40]:
        print("  differs:", k)
    return 1 if bad else 0


def summary_fields(summ):
    if hasattr(summ, "as_dict"):
        d = summ.as_dict()
    else:
        d = {f[0]: getattr(summ, f[0]) for f in getattr(summ, "_fields_", [])}
    return {k: v for k, v in d.items() if isinstance(v, (int, float)) and "seconds" not in k and "time" not in k}


def dump(out_path):
    from tests import lm_rule_cases as L
    from tests import nonlinear_position_scenes as ps
    from tests import test_lm_rules_gpu as T
    from tests import test_nonlinear_positions_gpu as TP
    from tests import test_nonlinear_rotations_gpu as TR

    out = {}
    for case, rule in L.CASE_RULES:
        _, pair = case.critical(rule)
        for side in (0, 1):
            for k, r in enumerate(T.device(case, rule, **L.tolerances(rule, pair[side]))):
                tag = f"{case.name}/{rule}/{side}/{k}"
                out[tag + "/summary"] = np.array([r.success, r.termination_type, r.num_iterations, r.num_successful_steps], np.int64)
                out[tag + "/costs"] = np.array([r.initial_cost, r.final_cost])
                for j, p in enumerate(r.params):
                    out[f"{tag}/params{j}"] = p
                if r.trace is not None:
                    for name in ("cost", "gradient_max_norm", "step_norm", "radius", "accepted"):
                        out[f"{tag}/trace_{name}"] = np.array(getattr(r.trace, name))
        print("done", case.name, rule, flush=True)
    x, summ, trace = TR.device(TR.scene("n22_outliers"))
    out["nonlinear_rotations/x"], out["nonlinear_rotations/trace"] = np.array(x), np.array(trace)
    for k, v in summary_fields(summ).items():
        out["nonlinear_rotations/summary_" + k] = np.array(v)
    name = TP.SHORT[0]
    x, pts, summ, trace = TP.device(name)
    out["nonlinear_positions/x"], out["nonlinear_positions/trace"] = np.array(x), np.array(trace)
    if pts is not None:
        out["nonlinear_positions/points"] = np.array(pts)
    for k, v in summary_fields(summ).items():
        out["nonlinear_positions/summary_" + k] = np.array(v)
    print("done nonlinear", name, flush=True)
    np.savez(out_path, **out)
    print(f"{len(out)} arrays -> {out_path}")
    return 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    sys.exit(dump(sys.argv[1]))
