"""The launches of a run, from the kernel trace rocprofv3 wrote as CSV: per queue (numbered by first appearance) the kernels in start order, a line
each of `queue  kernel  grid  workgroup`.  Two builds launch the same when these lists are equal:

    rocprofv3 --kernel-trace --output-format csv -d TRACE_DIR -- python scripts/frame_stage_ledger.py ledger.json
    python scripts/frame_stage_launches.py list TRACE_DIR > launches.txt
    python scripts/frame_stage_launches.py compare A.txt B.txt      # per queue in order, then as a multiset; exit status 1 if the multisets differ
"""
import collections
import csv
import glob
import os
import sys


def launches(trace_dir):
    rows = []
    for path in sorted(glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)):
        with open(path, newline="") as f:
            rows += list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    queues = {}
    out = []
    for r in rows:
        q = queues.setdefault(r["Queue_Id"], len(queues))
        name = r["Kernel_Name"].split("(")[0]
        grid = "x".join(r["Grid_Size_" + a] for a in "XYZ")
        wg = "x".join(r["Workgroup_Size_" + a] for a in "XYZ")
        out.append(f"{q}  {name}  {grid}  {wg}")
    return out


def compare(a, b):
    la, lb = [open(p).read().splitlines() for p in (a, b)]
    per_queue = lambda ls: {q: [l for l in ls if l.split("  ")[0] == q] for q in sorted({l.split("  ")[0] for l in ls})}
    in_order = per_queue(la) == per_queue(lb)
    strip = lambda ls: collections.Counter(l.split("  ", 1)[1] for l in ls)
    ca, cb = strip(la), strip(lb)
    print(f"{a}: {len(la)} launches, {b}: {len(lb)} launches")
    print("per queue, in start order: " + ("equal" if in_order else "different"))
    print("as a multiset of (kernel, grid, workgroup): " + ("equal" if ca == cb else "different"))
    for k in sorted(set(ca) | set(cb)):
        if ca[k] != cb[k]:
            print(f"  {ca[k]:6d} {cb[k]:6d}  {k}")
    return ca == cb


if __name__ == "__main__":
    if sys.argv[1] == "list":
        print("\n".join(launches(sys.argv[2])))
    else:
        sys.exit(0 if compare(sys.argv[2], sys.argv[3]) else 1)
