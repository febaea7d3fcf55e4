#!/usr/bin/env python3
"""Summary of two `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python3 bench.py --gpus 1 --steps 20
--warmup 3` runs (no counters), this tree's and the parent library's (LJMD_LIBRARY): the step's kernels, and per re-sort
the launches, their summed duration and the span from the first launch's start to the last one's end
(profiles/resort_class_kernel_trace.txt).  usage: resort_class_trace.py DIR_NEW DIR_PARENT"""
import csv
import sys
from pathlib import Path

STEP_KERNELS = ("pair_n3", "reduce_forces", "kick_", "fold_partials", "finalize", "tile_class", "drift_kick", "tile_boxes")
RESORT_KERNELS = ("rocprim", "kd_keys", "kd_finish", "iota_kernel", "gather", "copyBuffer")


def load(d):
    f = next(Path(d).rglob("*kernel_trace.csv"))
    out = [(r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in csv.DictReader(open(f))]
    out.sort(key=lambda x: x[1])
    return out


def short(name):
    name = name.split("(")[0].replace("void ", "").replace("ljmdk::", "")
    return "rocprim (library sort)" if "rocprim" in name else name


def avg(v):
    return sum(v) / len(v)


for tag, d in zip(("new", "parent"), sys.argv[1:3]):
    k = load(d)
    print(f"== {tag}: rocprofv3 --kernel-trace --stats -- python3 bench.py --gpus 1 --steps 20 --warmup 3 (no counters)")
    stats = {}
    for n, s, e in k:
        stats.setdefault(short(n), []).append((e - s) / 1e6)
    for n, v in sorted(stats.items(), key=lambda x: -sum(x[1])):
        if any(w in n for w in STEP_KERNELS + RESORT_KERNELS):
            print(f"  {n:45s} calls {len(v):4d}  avg {avg(v):9.4f} ms  min {min(v):9.4f}  max {max(v):9.4f}")
    # a re-sort: a run of its kernels with no kernel of a step in between, the library sort among them
    groups, cur = [], []
    for n, s, e in k:
        if any(w in n for w in RESORT_KERNELS):
            cur.append((n, s, e))
        elif any(w in n for w in STEP_KERNELS) and cur:
            groups.append(cur)
            cur = []
    if cur:
        groups.append(cur)
    groups = [g for g in groups if any("kd_keys" in n or "kd_finish" in n for n, _s, _e in g)]
    print(f"  re-sorts: {len(groups)}")
    for g in groups:
        lib = sum("rocprim" in n for n, _s, _e in g)
        print(f"    launches {len(g):4d} (library sort {lib:4d})  summed duration {sum(e - s for _n, s, e in g) / 1e6:7.4f} ms"
              f"  first start to last end {(g[-1][2] - g[0][1]) / 1e6:7.4f} ms")
    starts = sorted(s for n, s, e in k if "pair_n3_kernel" in n)
    starts = [s for j, s in enumerate(starts) if j == 0 or s - starts[j - 1] > 1e6]      # one per step: the first launch
    period = sorted((b - a) / 1e6 for a, b in zip(starts, starts[1:]))
    print(f"  pair launch start to the next step's, ms: avg {avg(period):.4f} median {period[len(period) // 2]:.4f} min {period[0]:.4f}")
