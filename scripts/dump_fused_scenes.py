"""dump_fused_scenes.py OUT_DIR -- the reduced camera system and the parameters of a five-iteration solve of every scene of
tests/test_fused_lds_batches_gpu.py and tests/test_fused_plan_shapes_gpu.py, one .npy per array, for comparing two builds of
the library byte for byte (a change of k_lin_schur / k_backsub_runs that only reschedules loads must not move a bit):

    THEIA_HIP_LIBRARY=/path/to/parent/libtheia_hip.so python scripts/dump_fused_scenes.py parent_dir
    python scripts/dump_fused_scenes.py branch_dir
    python scripts/dump_fused_scenes.py --compare parent_dir branch_dir

One process per library.  --compare prints a JSON summary and exits 1 on any difference (np.array_equal per array)."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def dump(out_dir):
    from pytheiasfm_amd import ba
    from tests import test_fused_lds_batches_gpu as B
    from tests import test_fused_plan_shapes_gpu as S

    os.makedirs(out_dir, exist_ok=True)
    scenes = [("batch_" + n, B.build_scene, n, B.SCENES[n]["run_obs"]) for n in sorted(B.SCENES)]
    scenes += [("shape_%d" % t, S.build_scene, t, None) for t in sorted(S.SCENES)]
    for tag, build, key, run_obs in scenes:
        if run_obs:
            os.environ["THEIA_HIP_FUSED_RUN_OBS"] = str(run_obs)
        p = build(key)
        o = ba.default_options()
        with ba.BaHandle(p.copy(), o) as h:
            Sm, rhs = h.reduced_system(1e4)
        o.max_num_iterations = 5
        q = p.copy()
        s, tr = ba.solve(q, o)
        os.environ.pop("THEIA_HIP_FUSED_RUN_OBS", None)
        for name, a in (("S", Sm), ("rhs", rhs), ("cam_ext", q.cam_ext), ("points", q.points), ("intrinsics", q.intrinsics),
                        ("cost", np.array(tr.cost[: tr.size])), ("accepted", np.array(tr.accepted[: tr.size]))):
            np.save(os.path.join(out_dir, "%s__%s.npy" % (tag, name)), np.ascontiguousarray(a))
        print("dumped", tag, s.num_iterations, flush=True)
    return 0


def compare(a_dir, b_dir):
    fa = sorted(f for f in os.listdir(a_dir) if f.endswith(".npy"))
    fb = sorted(f for f in os.listdir(b_dir) if f.endswith(".npy"))
    differ = sorted(set(fa) ^ set(fb))
    for f in sorted(set(fa) & set(fb)):
        x, y = np.load(os.path.join(a_dir, f)), np.load(os.path.join(b_dir, f))
        if x.dtype != y.dtype or not np.array_equal(x, y) or x.tobytes() != y.tobytes():
            differ.append(f)
    print(json.dumps({"arrays": len(fa), "arrays_other": len(fb), "differ": differ}))
    return 1 if differ else 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    sys.exit(dump(sys.argv[1]))
