#!/usr/bin/env python3
"""The measurements behind LJMD_REDUCE_SPLIT (MEASUREMENTS R6.1), each a table on stdout.

  ab    --parent-lib PATH [--runs 5]   `bench.py --gpus 1 --steps 20 --warmup 3` alternating between the library of the
                                       parent commit (LJMD_LIBRARY=PATH) and this tree's, one line per run, then the
                                       verdict: the change counts only if this tree's SLOWEST ms_per_step is below the
                                       parent's FASTEST of the same session (profiles/reduce_split_ab.txt)
  sweep [--reps 2]                     deferred share at n = 262144 (0 = off, then S/16, S/8, S/4 and neighbours), on / off
                                       at the sizes around the threshold and above it (profiles/reduce_split_sweep.txt)

Every run is a fresh process under its own time limit; the first failure ends the session."""
import argparse
import json
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def bench(env_extra, n=None, steps=20):
    env = {k: v for k, v in os.environ.items() if not k.startswith("LJMD_")}
    env.update(env_extra)
    cmd = ["timeout", "-k", "10", "240", sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "3"]
    if n is not None:
        cmd += ["--particles", str(n)]
    p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True)
    if p.returncode != 0:
        sys.exit("bench.py failed (%d):\n%s\n%s" % (p.returncode, p.stdout[-2000:], p.stderr[-4000:]))
    line = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    r = line["roofline"]
    return {"ms_per_step": line["ms_per_step"], "kernel_ms_avg": r["kernel_ms_avg"], "kernel_ms_min": r["kernel_ms_min"],
            "reduce_ms": r["reduce_kick_finalize_ms_avg"], "etot_last": line["energy_check"]["etot_last"]}


def row(tag, m):
    print("%-22s ms_per_step %8.4f  kernel_ms_avg %8.4f  kernel_ms_min %8.4f  reduce_kick_finalize_ms_avg %.4f  "
          "step-kernel_min %.4f" % (tag, m["ms_per_step"], m["kernel_ms_avg"], m["kernel_ms_min"], m["reduce_ms"],
                                    m["ms_per_step"] - m["kernel_ms_min"]), flush=True)


def ab(args):
    print("# python bench.py --gpus 1 --steps 20 --warmup 3, alternating parent / new, one card, one session")
    runs = {"parent": [], "new": []}
    for k in range(args.runs):
        for tag, env in (("parent", {"LJMD_LIBRARY": args.parent_lib}), ("new", {})):
            m = bench(env)
            runs[tag].append(m)
            row("%s run %d" % (tag, k + 1), m)
    for tag, ms in runs.items():
        v = [m["ms_per_step"] for m in ms]
        gap = [m["ms_per_step"] - m["kernel_ms_min"] for m in ms]
        print("%-6s ms_per_step fastest %.4f slowest %.4f mean %.4f | ms_per_step - kernel_ms_min: mean %.4f (mark: 0.5)"
              % (tag, min(v), max(v), sum(v) / len(v), sum(gap) / len(gap)))
    slowest_new = max(m["ms_per_step"] for m in runs["new"])
    fastest_parent = min(m["ms_per_step"] for m in runs["parent"])
    print("new slowest %.4f %s parent fastest %.4f: %s" % (slowest_new, "<" if slowest_new < fastest_parent else ">=",
                                                           fastest_parent, "KEPT" if slowest_new < fastest_parent else "NOT A GAIN"))
    return 0 if slowest_new < fastest_parent else 1


def sweep(args):
    print("# bench.py --gpus 1 --steps 20 --warmup 3 --particles n; LJMD_REDUCE_SPLIT = slices of the pair kernel's S in the second launch")
    for n, S, ks in ((262144, 103, (0, 6, 10, 13, 16, 20, 26, 34)), (131072, 129, (0, 16, 32)), (65536, 65, (0, 8, 16))):
        for rep in range(args.reps):
            for k in ks:
                row("n %d S %d split %d" % (n, S, k), bench({"LJMD_REDUCE_SPLIT": str(k)}, n))
    for n, steps in ((524288, 20), (1048576, 10)):
        for rep in range(args.reps):
            row("n %d split 0" % n, bench({"LJMD_REDUCE_SPLIT": "0"}, n, steps))
            row("n %d default" % n, bench({}, n, steps))
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    a = sub.add_parser("ab")
    a.add_argument("--parent-lib", required=True)
    a.add_argument("--runs", type=int, default=5)
    s = sub.add_parser("sweep")
    s.add_argument("--reps", type=int, default=2)
    args = ap.parse_args()
    sys.exit(ab(args) if args.cmd == "ab" else sweep(args))
