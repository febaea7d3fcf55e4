#!/usr/bin/env python3
"""Summary of two `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python3 bench.py --gpus 1 --steps 20
--warmup 3` runs (no counters), this tree's and the parent library's (LJMD_LIBRARY): per-kernel durations of the step's
kernels, and for this tree where the first phase of the slab reduction lies relative to the two pair launches of its step
(profiles/reduce_split_kernel_trace.txt).  usage: reduce_split_trace.py DIR_NEW DIR_PARENT"""
import csv
import sys
from pathlib import Path


def load(d):
    f = next(Path(d).rglob("*kernel_trace.csv"))
    out = [(r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Queue_Id"]) for r in csv.DictReader(open(f))]
    out.sort(key=lambda x: x[1])
    return out


def short(name):
    return name.split("(")[0].replace("void ", "").replace("ljmdk::", "")


def avg(v):
    return sum(v) / len(v)


STEP_KERNELS = ("pair_n3", "reduce_forces", "kick_", "fold_partials", "finalize", "tile_class", "drift_kick", "tile_boxes")
for tag, d in zip(("new", "parent"), sys.argv[1:3]):
    k = load(d)
    print(f"== {tag}: rocprofv3 --kernel-trace --stats -- python3 bench.py --gpus 1 --steps 20 --warmup 3 (no counters)")
    stats = {}
    for n, s, e, _q in k:
        stats.setdefault(short(n), []).append((e - s) / 1e6)
    for n, v in sorted(stats.items(), key=lambda x: -sum(x[1])):
        if any(w in n for w in STEP_KERNELS):
            print(f"  {n:45s} calls {len(v):4d}  avg {avg(v):9.4f} ms  min {min(v):9.4f}  max {max(v):9.4f}")
    pairs = [(s, e, q) for n, s, e, q in k if "pair_n3_kernel" in n]
    ph1 = [(s, e, q) for n, s, e, q in k if "reduce_forces_split_kernel<1>" in n]
    if ph1:
        rows = []
        for s, e, q in ph1:
            two = sorted((p for p in pairs if p[0] <= s), key=lambda p: -p[0])[:2]     # the two pair launches of this step
            first = next(p for p in two if p[2] == q)                                   # same queue as phase 1
            second = next(p for p in two if p[2] != q)
            rows.append(((first[1] - first[0]) / 1e6, (second[1] - second[0]) / 1e6, (second[0] - first[0]) / 1e6,
                         (s - first[1]) / 1e6, (e - second[1]) / 1e6, (min(e, second[1]) - s) / 1e6, (e - s) / 1e6,
                         (max(e, second[1]) - first[0]) / 1e6))
        names = ("first pair launch, duration", "second pair launch (side stream), duration", "second launch start - first launch start",
                 "phase-1 start - first launch end", "phase-1 end - second launch end", "phase 1 beside the second launch",
                 "phase 1, duration", "first launch start to the later of (second launch, phase 1) end")
        print(f"  per step ({len(rows)} steps), ms:")
        for j, nm in enumerate(names):
            col = [r[j] for r in rows]
            print(f"    {nm:66s} avg {avg(col):8.4f}  min {min(col):8.4f}  max {max(col):8.4f}")
        inside = sum(r[3] >= 0 and r[4] <= 0 for r in rows)
        print(f"    phase 1 entirely inside [first launch start, second launch end]: {inside} of {len(rows)} steps")
        starts = sorted(p[0] for p in pairs if p[2] == ph1[0][2])
    else:
        starts = sorted(p[0] for p in pairs)
    period = [(b - a) / 1e6 for a, b in zip(starts, starts[1:])]
    print(f"  pair launch start to the next step's, ms: avg {avg(period):.4f} min {min(period):.4f}")
