"""CPU: the lane-occupancy model of the fused BA plan (csrc/ba_plan_stats.h) on a hand-built plan of three runs
(tests/plan_occupancy_check.cpp), against counts written out by hand here."""
import json
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Four waves per workgroup, four tiles per sub-chunk; targets of W cameras in (la, lb) order: index la (la + 1) / 2 + lb.
#
# Run A (G = 1, two equal slices of 32 lanes, 6 targets; slots 0: cameras {0, 1}, 1: {0, 1, 2}, 2: {2}; stride 8):
#   wave 0 serves slots 0, 1: slot 0 has (0,0) (1,0) (1,1) = 3 of 6, slot 1 all 6; 2 x 26 slice lanes hold no target
#     -> runs: useful 9, sparsity 3, shape 52
#   wave 1 serves slots 2, 3: slot 2 has (2,2) = 1 of 6; slot 3 is past the last track: 26 + 32 lanes idle by shape
#     -> runs: useful 1, sparsity 5, shape 58
#   waves 2, 3: slots 4 .. 7, no track -> 2 skipped
#
# Run B (G = 2: waves 0, 2 own targets 0 .. 63, waves 1, 3 own 64 .. 77; slot 0: {0, 1}, slot 1: {11}; stride 2):
#   waves 0, 1 serve slot 0: targets 0, 1, 2 -> wave 0 runs (useful 3, sparsity 61, shape 0), wave 1 finds none: skipped
#   waves 2, 3 serve slot 1: target (11,11) = 77 -> wave 2 skipped, wave 3 runs (useful 1, sparsity 13, shape 50)
#
# Run C (G = 1, slices of 6, 3, 1 targets = 10 lanes, 54 lanes in no slice; slots 0: {0, 1, 2}, 1: {0, 1},
#        2: {0, a constant camera}, 3: {1, 2}, 4: empty; 5 slots; stride 12):
#   wave 0 serves slots 0, 1, 2: 6 of 6, 3 of 3, 1 of 1 -> runs: useful 10, sparsity 0, shape 54
#   wave 1 serves slots 3, 4, 5: slot 3 has (1,1) (2,1) (2,2) = 3 of 6; slot 4 empty (3 lanes), slot 5 past the end (1 lane)
#     -> runs: useful 3, sparsity 3, shape 58
#   waves 2, 3: skipped
EXPECTED = {
    #        steps skipped useful idle_shape idle_sparsity tracks observations
    "A": (2, 2, 10, 110, 8, 3, 6),
    "B": (2, 2, 4, 50, 74, 2, 3),
    "C": (2, 2, 13, 112, 3, 4, 9),
    "total": (6, 6, 27, 272, 85, 9, 18),
}


def test_issued_steps_of_a_hand_built_plan(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler found"
    exe = str(tmp_path / "plan_occupancy_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "pytheiasfm_amd", "csrc"),
                    os.path.join(ROOT, "tests", "plan_occupancy_check.cpp"), "-o", exe], check=True, timeout=120)
    r = subprocess.run([exe], timeout=60, capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-800:])
    got = {ln.split()[0]: tuple(int(x) for x in ln.split()[1:]) for ln in r.stdout.splitlines() if ln.strip()}
    assert got == EXPECTED
    for name, (steps, _, useful, shape, sparsity, _, _) in got.items():
        assert 64 * steps == useful + shape + sparsity, name
    # the JSON form of the same model (what THEIA_HIP_PLAN_STATS=<path> writes)
    js = json.loads(r.stderr)
    assert js["runs"] == 3 and js["total"]["steps_issued"] == 6 and js["total"]["lanes_useful"] == 27
    assert js["objective_steps"] == 6 + 3 * js["run_cost_steps"]
    assert len(js["run_rows"]) == 3 and len(js["run_rows"][0]) == len(js["run_columns"])
    assert [s["unequal_slices"] for s in js["by_shape"]] == [0, 0, 1]
