#!/usr/bin/env python3
"""Cost of the engine's resident g(r) (Engine.rdf_*, ljmd_rdf_*), measured in one process on one card.  One JSON line per
system size, also written to profiles/rdf_resident_rate.txt (--out PATH for another file).

The system is the bench workload's recipe (synthetic.make_config: rho = 0.8, rc = 0.49 L, jittered lattice), advanced
--steps steps (default 300) so that the tiles are between two re-sorts.  Then, alternating, --repeats times (default 5)
after one warm-up round, each figure reported as its minimum and its spread (max - min):

  resident_half_ms    ljmd_rdf_profile_read's kernel time (HIP events around the two launches) of one rdf_accumulate with
                      rmax = L / 2, and half_visited_fraction = tile pairs evaluated / considered
  resident_r5_ms      the same with rmax = 5.0, r5_visited_fraction
  stateless_half_ms   the route without the feature to the same integers: one blocking ljmd_rdf_histogram call on the
                      positions get_state returned (host clock around the call: upload, all-pairs kernel, download).
                      get_state itself -- what a driver without the feature pays first -- is reported as get_state_ms
  md_step_ms          one MD step of the same engine: wall time of verlet_steps(--step-batch, default 100) / that many

The histograms of the resident pass (rmax = L / 2) and of the stateless call must be equal; the tool fails otherwise.
segment_share = resident ms / (100 md_step_ms): one snapshot per output_interval = 100 segment.

Usage: rdf_resident_rate.py [--out PATH] [--steps K] [--repeats R] [--step-batch S] [n ...]   Default n: 4096 262144.
Measurement tool."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import ljmd_amd  # noqa: E402,F401
from ljmd_amd import Engine, analysis, synthetic  # noqa: E402

NBINS = 200


def spread(xs):
    return {"min": round(min(xs), 4), "spread": round(max(xs) - min(xs), 4)}


def resident(eng, rmax):
    eng.rdf_configure(NBINS, rmax)
    eng.rdf_accumulate()
    prof = eng.rdf_profile()                                 # waits for the device
    hist, count = eng.rdf_read()
    assert count == 1
    return prof, hist


def measure(n, steps, repeats, step_batch):
    p, r, v = synthetic.make_config(n)
    L = p.box_length
    half, r5 = 0.5 * L, 5.0
    with Engine(p) as eng:
        eng.set_state(r[0], r[1], r[2], v[0], v[1], v[2])
        eng.compute_forces()
        eng.advance(steps)
        t_half, t_r5, t_stateless, t_get, t_step = [], [], [], [], []
        frac_half = frac_r5 = None
        for rep in range(repeats + 1):                       # round 0 warms every path up
            prof, hist_half = resident(eng, half)
            a = prof["kernel_ms"]
            frac_half = prof["tile_pairs_visited"] / prof["tile_pairs_total"]
            prof, _ = resident(eng, r5)
            b = prof["kernel_ms"]
            frac_r5 = prof["tile_pairs_visited"] / prof["tile_pairs_total"]
            t0 = time.perf_counter()
            x, y, z = eng.get_state(("r",))["r"]
            t1 = time.perf_counter()
            host = np.zeros(NBINS, dtype=np.uint64)
            analysis.rdf_histogram(x, y, z, L, NBINS, half, host)
            t2 = time.perf_counter()
            assert np.array_equal(host, hist_half), "resident and stateless histograms differ"
            t3 = time.perf_counter()
            eng.advance(step_batch)
            t4 = time.perf_counter()
            if rep:
                t_half.append(a)
                t_r5.append(b)
                t_get.append(1e3 * (t1 - t0))
                t_stateless.append(1e3 * (t2 - t1))
                t_step.append(1e3 * (t4 - t3) / step_batch)
    step = min(t_step)
    return {"n": n, "box_length": round(L, 4), "nbins": NBINS, "steps_before": steps, "repeats": repeats,
            "resident_half_ms": spread(t_half), "half_visited_fraction": round(frac_half, 4),
            "resident_r5_ms": spread(t_r5), "r5_visited_fraction": round(frac_r5, 4),
            "stateless_half_ms": spread(t_stateless), "get_state_ms": spread(t_get),
            "md_step_ms": spread(t_step),
            "resident_half_over_stateless": round(min(t_half) / min(t_stateless), 4),
            "segment_share_half": round(min(t_half) / (100.0 * step), 5),
            "segment_share_r5": round(min(t_r5) / (100.0 * step), 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "rdf_resident_rate.txt")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--step-batch", type=int, default=100)
    ap.add_argument("n", type=int, nargs="*", default=[4096, 262144])
    a = ap.parse_args()
    a.out.parent.mkdir(parents=True, exist_ok=True)
    with open(a.out, "w") as f:
        for n in a.n:
            line = json.dumps(measure(n, a.steps, a.repeats, a.step_batch))
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()


if __name__ == "__main__":
    main()
