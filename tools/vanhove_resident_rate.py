#!/usr/bin/env python3
"""Cost of the engine's resident van Hove self-correlation (Engine.vanhove_*, ljmd_vanhove_*), measured in one process
on one card against two yardsticks of the same handle: ljmd_tcf_accumulate with the same (max_lag, stride), and one MD
step.  One JSON line per (system size, live origins, nbins), also written to profiles/vanhove_resident_rate.txt (--out
PATH for another file).

The system is the bench workload's recipe (synthetic.make_config: rho = 0.8, rc = 0.49 L, jittered lattice), advanced
--steps steps (default 300).  For `live` live origins both features are configured with max_lag = 2 live - 1 and origin
stride 2 (`live` ring slots each) and 2 live snapshots are taken ONE MD STEP APART, so that the displacements -- and with
them the bins the LDS atomics hit -- are those of a run, from 1 to 2 live - 1 steps; from then on every snapshot with an
odd number meets exactly `live` origins.  rmax = --rmax (default 3 sigma).  Then, alternating the order of the two
accumulates, --repeats rounds (default 5) after one warm-up round, each figure reported as its minimum and its spread
(max - min):

  vanhove_ms     ljmd_vanhove_profile_read's kernel time (HIP events around the three launches) of one accumulate that
                 visits `live` origins (origins_live is checked); gbytes_per_s = 24 n_pad live / that time
  tcf_ms         the same of ljmd_tcf_accumulate on the same state (48 n_pad live bytes)
  step_ms        one MD step of the handle: host clock around 10 blocking steps, divided by 10
  get_state_ms   the route the feature replaces, per sampling instant: get_state of ru to the host (host clock) ...
  numpy_bin_ms   ... and the numpy binning of ONE (origin, lag): differences, lengths, np.bincount over n particles;
                 host_route_ms = get_state_ms + live numpy_bin_ms is that route's cost of the same snapshot

ratio_to_tcf = vanhove_ms / tcf_ms, ratio_to_step = vanhove_ms / step_ms.  No pass mark.

Usage: vanhove_resident_rate.py [--out PATH] [--steps K] [--repeats R] [--live 16 128 512] [--nbins 128 1024] [n ...]
Default n: 4096 65536 262144.  Measurement tool."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import ljmd_amd  # noqa: E402,F401
from ljmd_amd import Engine, synthetic  # noqa: E402


def spread(xs):
    return {"min": round(min(xs), 4), "spread": round(max(xs) - min(xs), 4)}


def both(eng, vanhove_first):
    if vanhove_first:
        eng.vanhove_accumulate()
        eng.tcf_accumulate()
    else:
        eng.tcf_accumulate()
        eng.vanhove_accumulate()


def resident_once(eng, live, vanhove_first):
    """two snapshots a step apart; -> kernel ms (van Hove, MSD / VACF) of the odd-numbered one, which meets `live`
    origins"""
    eng.verlet_steps(1)
    both(eng, vanhove_first)                                 # even number: live - 1 origins, stored
    eng.verlet_steps(1)
    both(eng, vanhove_first)
    pv, pt = eng.vanhove_profile(), eng.tcf_profile()        # wait for the device
    assert pv["origins_live"] == live and pt["origins_live"] == live, (pv, pt)
    return pv["kernel_ms"], pt["kernel_ms"]


def measure(eng, n, live, nbins, rmax, steps, repeats):
    n_pad = (n + 1023) // 1024 * 1024
    eng.tcf_configure(2 * live - 1, 2)
    eng.vanhove_configure(2 * live - 1, 2, nbins, rmax)
    for _ in range(2 * live):
        eng.verlet_steps(1)
        both(eng, False)
    t_vh, t_tcf, t_step, t_get, t_bin = [], [], [], [], []
    ru0 = np.stack(eng.get_state(("ru",))["ru"])
    for rep in range(repeats + 1):                           # round 0 warms every path up
        a, b = resident_once(eng, live, rep % 2 == 1)
        t0 = time.perf_counter()
        eng.verlet_steps(10)
        t1 = time.perf_counter()
        ru = np.stack(eng.get_state(("ru",))["ru"])
        t2 = time.perf_counter()
        d = ru - ru0
        r = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        hist = np.bincount(np.minimum((r / (rmax / nbins)).astype(np.int64), nbins), minlength=nbins + 1)
        t3 = time.perf_counter()
        assert hist.sum() == n
        if rep:
            t_vh.append(a)
            t_tcf.append(b)
            t_step.append(1e2 * (t1 - t0))
            t_get.append(1e3 * (t2 - t1))
            t_bin.append(1e3 * (t3 - t2))
    hist, _, _, counts, _ = eng.vanhove_read()
    overflow = float(hist[:, nbins].sum()) / float(hist.sum())
    busiest = float(hist[2 * live - 1].max()) / float(hist[2 * live - 1].sum())      # share of the fullest bin at the longest lag
    eng.tcf_configure(0)
    eng.vanhove_configure(0)
    vh, tcf, step = min(t_vh), min(t_tcf), min(t_step)
    return {"n": n, "live_origins": live, "nbins": nbins, "rmax": rmax, "steps_before": steps, "repeats": repeats,
            "vanhove_ms": spread(t_vh), "gbytes_per_s": round(24.0 * n_pad * live / (vh * 1e-3) / 1e9, 1),
            "tcf_ms": spread(t_tcf), "step_ms": spread(t_step), "ratio_to_tcf": round(vh / tcf, 3),
            "ratio_to_step": round(vh / step, 3), "get_state_ms": spread(t_get), "numpy_bin_ms": spread(t_bin),
            "host_route_ms": round(min(t_get) + live * min(t_bin), 3), "overflow_fraction": round(overflow, 4),
            "fullest_bin_share_longest_lag": round(busiest, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "vanhove_resident_rate.txt")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--live", type=int, nargs="+", default=[16, 128, 512])
    ap.add_argument("--nbins", type=int, nargs="+", default=[128, 1024])
    ap.add_argument("--rmax", type=float, default=3.0)
    ap.add_argument("n", type=int, nargs="*", default=[4096, 65536, 262144])
    a = ap.parse_args()
    a.out.parent.mkdir(parents=True, exist_ok=True)
    with open(a.out, "w") as f:
        for n in a.n:
            p, r, v = synthetic.make_config(n)
            with Engine(p) as eng:
                eng.set_state(r[0], r[1], r[2], v[0], v[1], v[2])
                eng.compute_forces()
                eng.advance(a.steps)
                for live in a.live:
                    for nbins in a.nbins:
                        line = json.dumps(measure(eng, n, live, nbins, a.rmax, a.steps, a.repeats))
                        print(line, flush=True)
                        f.write(line + "\n")
                        f.flush()


if __name__ == "__main__":
    main()
