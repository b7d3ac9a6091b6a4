#!/usr/bin/env python3
"""Condenses a rocprofv3 --kernel-trace --stats directory of one bench.py run (tools/trace_overlap.sh): per kernel of the last `steps`
steps the number of dispatches and the average duration; for the pyramid-levels dispatches (pyr_strip_kernel, pyr_down_kernel) the share
of their time that lies inside the interval of a motion-search dispatch and of a transform dispatch; the timeline of the last three steps.
usage: trace_overlap.py <raw dir> <out.txt> [bench line]"""
import csv
import glob
import json
import os
import sys

raw, out = sys.argv[1], sys.argv[2]
bench = json.loads(sys.argv[3]) if len(sys.argv) > 3 and sys.argv[3].strip().startswith("{") else {}
rows = []
for p in glob.glob(os.path.join(raw, "**", "*kernel_trace.csv"), recursive=True):
    rows += list(csv.DictReader(open(p)))
assert rows, f"no *kernel_trace.csv under {raw}"


def short(name):
    return name.split("(")[0].replace("void svc::", "").replace("svc::", "")


k = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"]), r.get("Queue_Id", "?")) for r in rows if "svc::" in r["Kernel_Name"]]
k.sort()
# the front-of-step transform: one dispatch per step in the one-pass order (the redo of the foreground tiles is the same kernel, but short)
fronts = [i for i, r in enumerate(k) if r[2].startswith("dct_kernel") and r[1] - r[0] > 500000]
steps = 16
assert len(fronts) > steps + 1, "too few steps in the trace"
lo, hi = k[fronts[-steps - 1]][0], k[fronts[-1]][0]  # the last `steps` whole steps, transform start to transform start
win = [r for r in k if lo <= r[0] < hi]


def inside(a, others):
    """ns of interval a covered by the union of `others` (sorted, non-overlapping among themselves: one stream)."""
    return sum(max(0, min(a[1], o[1]) - max(a[0], o[0])) for o in others)


search = [r for r in win if r[2].startswith("hbma")]
front = [k[i] for i in fronts]
levels = [r for r in win if r[2].startswith("pyr_strip") or r[2].startswith("pyr_down")]
with open(out, "w") as f:
    if bench:
        f.write(f"bench line: ms_per_step {bench.get('ms_per_step'):.4f}, kernel_ms_per_step {bench.get('kernel_ms_per_step')}\n")
    f.write(f"last {steps} steps of the trace: {(hi - lo) / steps / 1e6:.4f} ms per step (transform start to transform start)\n\n")
    f.write("kernel                              dispatches  avg_us\n")
    names = sorted({r[2] for r in win}, key=lambda n: -sum(r[1] - r[0] for r in win if r[2] == n))
    for n in names:
        d = [r[1] - r[0] for r in win if r[2] == n]
        f.write(f"{n[:34]:34s} {len(d):10d} {sum(d) / len(d) / 1e3:8.1f}\n")
    tot = sum(r[1] - r[0] for r in levels)
    f.write(f"\npyramid-levels dispatches: {len(levels)}, {tot / steps / 1e3:.1f} us per step; of that inside a motion-search dispatch "
            f"{sum(inside(r, search) for r in levels) / max(tot, 1) * 100:.1f} %, inside a transform dispatch "
            f"{sum(inside(r, front) for r in levels) / max(tot, 1) * 100:.1f} %\n")
    f.write("\ntimeline of the last three steps\nstart_us   end_us   dur_us queue kernel\n")
    t0 = k[fronts[-4]][0]
    for r in k:
        if t0 <= r[0] < hi:
            f.write(f"{(r[0] - t0) / 1e3:8.1f} {(r[1] - t0) / 1e3:8.1f} {(r[1] - r[0]) / 1e3:8.1f} q{r[3]} {r[2]}\n")
print(open(out).read())
