#!/usr/bin/env python3
"""A/B of the flagship line for the re-sort finishing kernel and the narrower tile_class grid (MEASUREMENTS R9).

  resort_class_ab.py --parent-lib PATH [--runs 5]

`bench.py --gpus 1 --steps 20 --warmup 3` alternating between the library of the parent commit (LJMD_LIBRARY=PATH) and
this tree's, one card, one session, one line per run; then per arm the mean and the standard deviation of ms_per_step,
and the verdict: a step gain is claimed only if the means differ by more than three times the larger standard deviation
(profiles/resort_class_ab.txt).  Every run is a fresh process under its own time limit; the first failure ends the session."""
import argparse
import statistics
import sys

from reduce_split_ab import bench


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--runs", type=int, default=5)
    args = ap.parse_args()
    print("# python bench.py --gpus 1 --steps 20 --warmup 3, alternating parent / new, one card, one session")
    runs = {"parent": [], "new": []}
    for k in range(args.runs):
        for tag, env in (("parent", {"LJMD_LIBRARY": args.parent_lib}), ("new", {})):
            m = bench(env)
            runs[tag].append(m)
            print("%-14s ms_per_step %8.4f  kernel_ms_avg %8.4f  kernel_ms_min %8.4f  ms_per_step - kernel_ms_avg %.4f"
                  % ("%s run %d" % (tag, k + 1), m["ms_per_step"], m["kernel_ms_avg"], m["kernel_ms_min"],
                     m["ms_per_step"] - m["kernel_ms_avg"]), flush=True)
    stat = {}
    for tag, ms in runs.items():
        v = [m["ms_per_step"] for m in ms]
        rest = [m["ms_per_step"] - m["kernel_ms_avg"] for m in ms]
        stat[tag] = (statistics.mean(v), statistics.stdev(v), statistics.mean(rest), statistics.stdev(rest))
        print("%-6s ms_per_step mean %.4f sd %.4f (min %.4f max %.4f) | ms_per_step - kernel_ms_avg mean %.4f sd %.4f"
              % (tag, stat[tag][0], stat[tag][1], min(v), max(v), stat[tag][2], stat[tag][3]))
    for what, k in (("ms_per_step", 0), ("ms_per_step - kernel_ms_avg", 2)):
        diff = stat["parent"][k] - stat["new"][k]
        sd = max(stat["parent"][k + 1], stat["new"][k + 1])
        print("%s: parent - new = %.4f ms, 3 x larger sd = %.4f: %s"
              % (what, diff, 3 * sd, "GAIN" if diff > 3 * sd else "NO GAIN CLAIMED"))
    return 0


if __name__ == "__main__":
    sys.exit(main())
