#!/usr/bin/env python3
"""Cost of the engine's resident heat flux (Engine.heatflux_*, ljmd_heatflux_*), measured in one process on one card.
One JSON line per (system size, cutoff), also written to profiles/heatflux_resident_rate.txt (--out PATH for another
file).

The system is the bench workload's recipe (synthetic.make_config: rho = 0.8, jittered lattice) with rc = 0.49 L and with
rc = 2.5, advanced --steps steps (default 300) so that the tiles are between two re-sorts.  Then, alternating, --repeats
times (default 5) after one warm-up round, each figure reported as its minimum and its spread (max - min):

  accumulate_ms         ljmd_heatflux_profile_read's kernel time (HIP events around the four launches) of one
                        heatflux_accumulate, tile_pairs_visited of its walk and visited_fraction = evaluated / considered
  stress_accumulate_ms  the yardstick: the same handle's stress_accumulate on the same state, timed the same way
  md_step_ms            the other yardstick, one MD step of the same handle: wall time of --step-batch (default 100)
                        enqueued steps / that many
  segment_plain_ms      wall time of one enqueued --step-batch segment, collected
  segment_heatflux_ms   the same with one heatflux_accumulate enqueued behind the segment, read with the records

accumulate_over_stress = accumulate_ms / stress_accumulate_ms and accumulate_over_step = accumulate_ms / md_step_ms, of
the minima.

Usage: heatflux_resident_rate.py [--out PATH] [--steps K] [--repeats R] [--step-batch S] [n ...]
Default n: 4096 65536 262144.  Measurement tool."""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import ljmd_amd  # noqa: E402,F401
from ljmd_amd import Engine, md_types, synthetic  # noqa: E402


def spread(xs):
    return {"min": round(min(xs), 4), "spread": round(max(xs) - min(xs), 4)}


def measure(n, rc, steps, repeats, step_batch):
    p, r, v = synthetic.make_config(n)
    L = p.box_length
    rc = 0.49 * L if rc is None else rc
    p = md_types.init_params(n, L, p.dt, rc)
    with Engine(p) as eng:
        eng.set_state(r[0], r[1], r[2], v[0], v[1], v[2])
        eng.compute_forces()
        eng.advance(steps)
        eng.heatflux_configure(4 * (repeats + 1))
        eng.stress_configure(2 * (repeats + 1))
        t_acc, t_stress, t_plain, t_flux = [], [], [], []
        prof = None
        for rep in range(repeats + 1):                       # round 0 warms every path up
            eng.heatflux_accumulate()
            prof = eng.heatflux_profile()                    # waits for the device
            eng.stress_accumulate()
            sprof = eng.stress_profile()
            t0 = time.perf_counter()
            eng.enqueue_steps(step_batch)
            eng.collect_steps(step_batch)
            t1 = time.perf_counter()
            eng.enqueue_steps(step_batch)
            eng.heatflux_accumulate()
            eng.collect_steps(step_batch)
            eng.heatflux_read()
            t2 = time.perf_counter()
            if rep:
                t_acc.append(prof["kernel_ms"])
                t_stress.append(sprof["kernel_ms"])
                t_plain.append(1e3 * (t1 - t0))
                t_flux.append(1e3 * (t2 - t1))
    step = min(t_plain) / step_batch
    return {"n": n, "box_length": round(L, 4), "rc": round(rc, 4), "steps_before": steps, "repeats": repeats,
            "step_batch": step_batch,
            "accumulate_ms": spread(t_acc), "tile_pairs_visited": prof["tile_pairs_visited"],
            "visited_fraction": round(prof["tile_pairs_visited"] / prof["tile_pairs_total"], 4),
            "stress_accumulate_ms": spread(t_stress), "accumulate_over_stress": round(min(t_acc) / min(t_stress), 3),
            "md_step_ms": round(step, 5), "accumulate_over_step": round(min(t_acc) / step, 3),
            "segment_plain_ms": spread(t_plain), "segment_heatflux_ms": spread(t_flux),
            "steps_per_s_plain": round(1e3 * step_batch / min(t_plain), 2),
            "steps_per_s_heatflux": round(1e3 * step_batch / min(t_flux), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "heatflux_resident_rate.txt")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--step-batch", type=int, default=100)
    ap.add_argument("n", type=int, nargs="*", default=[4096, 65536, 262144])
    a = ap.parse_args()
    a.out.parent.mkdir(parents=True, exist_ok=True)
    with open(a.out, "w") as f:
        for n in a.n:
            for rc in (None, 2.5):
                line = json.dumps(measure(n, rc, a.steps, a.repeats, a.step_batch))
                print(line, flush=True)
                f.write(line + "\n")
                f.flush()


if __name__ == "__main__":
    main()
