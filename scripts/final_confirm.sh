#!/bin/bash
# GPU box: the round's last check on the committed tree -- clean rebuild by build(), smoke(), the full bench line,
# pytest -m gpu -- summarised as <output directory>/final_confirm.json (copied to profiles/<tag>_final_confirm.json).
# usage: final_confirm.sh <output directory>
set -u
R="${GRAFT_REPO_ROOT:-/root/repo}"
OUT="$(realpath -m "${1:?usage: final_confirm.sh <output directory>}")"
cd "$R"; mkdir -p "$OUT"
rm -rf pytheiasfm_amd/csrc/_obj pytheiasfm_amd/libtheia_hip.so
python -c "import __graft_entry__ as g; g.build()" > "$OUT/confirm_build.log" 2>&1; brc=$?
python -c "import __graft_entry__ as g; g.smoke()" > "$OUT/confirm_smoke.log" 2>&1; src=$?
timeout 900 python bench.py --full > "$OUT/confirm_bench.json" 2> "$OUT/confirm_bench.err"
timeout 3000 python -m pytest tests -q -m gpu > "$OUT/confirm_tests.log" 2>&1
python - "$brc" "$src" "$OUT" <<'PY'
import json, os, sys
out_dir = sys.argv[3]
line = open(os.path.join(out_dir, "confirm_bench.json")).read().strip().splitlines()[-1]
tests = [l for l in open(os.path.join(out_dir, "confirm_tests.log")).read().splitlines() if " passed" in l or " failed" in l]
out = {"what": "clean rebuild by build(), smoke(), bench.py --full, pytest -m gpu on a fresh MI355X box", "build_rc": int(sys.argv[1]),
       "smoke_rc": int(sys.argv[2]), "gpu_tests": tests[-1] if tests else "no summary line", "bench_line": json.loads(line)}
json.dump(out, open(os.path.join(out_dir, "final_confirm.json"), "w"), indent=1)
b = out["bench_line"]
print(out["build_rc"], out["smoke_rc"], out["gpu_tests"], b["ms_per_step"], b["roofline"]["avg_launch_ms"], b["roofline"]["traffic"], b["roofline_k3"]["avg_solve_ms"])
PY
