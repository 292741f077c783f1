"""K3 dispatch by dispatch: the median duration of every K3 kernel of a steady-state LM iteration, in launch order, from a
rocprofv3 per-dispatch kernel trace (rocprofv3 --kernel-trace --output-format csv -- python bench.py --steps 16
--warmup 8 --full --no-cpu-baseline --no-ransac --no-c2).

  python scripts/k3_dispatch_table.py <..._kernel_trace.csv>

An iteration runs from one k_sp_clear to the next; the iterations with the most common K3 launch sequence (the C4
headline) are kept and the later half of them summarised."""
import collections
import csv
import re
import statistics
import sys

K3 = ("k_sp_symm", "k_sp_potrf_trsm", "k_sp_update", "k_sp_update_partial", "k_sp_update_reduce", "k_sp_back")


def main(path):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    names = []
    for r in rows:
        m = re.search(r"(k_\w+)", r["Kernel_Name"])
        names.append(m.group(1) if m else r["Kernel_Name"])
    starts = [i for i, n in enumerate(names) if n == "k_sp_clear"]
    its = [[i for i in range(a, b) if names[i] in K3] for a, b in zip(starts, starts[1:])]
    sig = lambda k3: tuple((names[i], int(rows[i]["Grid_Size_X"]) // int(rows[i]["Workgroup_Size_X"])) for i in k3)
    s0, count = collections.Counter(sig(k) for k in its if k).most_common(1)[0]
    sel = [k for k in its if k and sig(k) == s0]
    sel = sel[len(sel) // 2:]
    dur = lambda i: (int(rows[i]["End_Timestamp"]) - int(rows[i]["Start_Timestamp"])) * 1e-3
    print(f"{count} iterations with this sequence of {len(s0)} K3 launches, medians over the last {len(sel)}")
    total = 0.0
    for p, (name, wgs) in enumerate(s0):
        d = statistics.median(dur(k[p]) for k in sel)
        total += d
        print(f"{p:2d} {name:20s} {wgs:5d} workgroups {d:7.2f} us")
    span = statistics.median((int(rows[k[-1]]["End_Timestamp"]) - int(rows[k[0]]["Start_Timestamp"])) * 1e-3 for k in sel)
    print(f"sum {total:.1f} us, first start to last end {span:.1f} us")


if __name__ == "__main__":
    main(sys.argv[1])
