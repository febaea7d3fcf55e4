#!/usr/bin/env python3
"""Cost of the engine's resident current modes (Engine.current_*, ljmd_current_*), measured in one process on one card
beside its yardstick, the density modes' accumulate (ljmd_rhok_*) of the same handle and mode list.  One JSON line per
(system size, cutoff, number of modes), also written to profiles/current_resident_rate.txt (--out PATH for another file).

The system is the bench workload's recipe (synthetic.make_config: rho = 0.8, jittered lattice) with rc = 0.49 L (the
bench's cutoff) and with rc = 2.5 -- the accumulates do not depend on the cutoff, the MD step they are compared with
does -- advanced --steps steps (default 100) so that the tiles are between two re-sorts.  The mode list is random
triples with |n_a| <= 40 (the cost of a term does not depend on the mode).  Then, alternating, --repeats times (default
5) after one warm-up round, each figure reported as its minimum and its spread (max - min):

  current_accumulate_ms  ljmd_current_profile_read's kernel time (HIP events around the two launches) of one accumulate
  rhok_accumulate_ms     ljmd_rhok_profile_read's, for the same state and the same list
  md_step_ms             one MD step of the same handle: wall time of --step-batch (default 20) enqueued steps / that many

current_over_rhok = min current_accumulate_ms / min rhok_accumulate_ms; current_over_step = min current_accumulate_ms /
md_step_ms.

Usage: current_resident_rate.py [--out PATH] [--steps K] [--repeats R] [--step-batch S] [--modes M ...] [n ...]
Default n: 4096 65536 262144; default modes: 64 1024 4096.  Measurement tool."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import ljmd_amd  # noqa: E402,F401
from ljmd_amd import Engine, md_types, synthetic  # noqa: E402


def spread(xs):
    return {"min": round(min(xs), 4), "spread": round(max(xs) - min(xs), 4)}


def mode_list(count):
    return np.random.default_rng(count).integers(-40, 41, size=(count, 3)).astype(np.int32)


def measure(n, rc, counts, steps, repeats, step_batch):
    p, r, v = synthetic.make_config(n)
    L = p.box_length
    rc = 0.49 * L if rc is None else rc
    p = md_types.init_params(n, L, p.dt, rc)
    with Engine(p) as eng:
        eng.set_state(r[0], r[1], r[2], v[0], v[1], v[2])
        eng.compute_forces()
        eng.advance(steps)
        t_plain = []
        t_cur = {c: [] for c in counts}
        t_rhok = {c: [] for c in counts}
        for rep in range(repeats + 1):                       # round 0 warms every path up
            t0 = time.perf_counter()
            eng.enqueue_steps(step_batch)
            eng.collect_steps(step_batch)
            t1 = time.perf_counter()
            if rep:
                t_plain.append(1e3 * (t1 - t0))
            for c in counts:
                eng.rhok_configure(mode_list(c), 1)
                eng.current_configure(mode_list(c), 1)
                eng.rhok_accumulate()
                eng.current_accumulate()
                rhok = eng.rhok_profile()                    # waits for the device
                cur = eng.current_profile()
                if rep:
                    t_rhok[c].append(rhok["kernel_ms"])
                    t_cur[c].append(cur["kernel_ms"])
        eng.rhok_configure(None, 0)
        eng.current_configure(None, 0)
    step = min(t_plain) / step_batch
    return [{"n": n, "rc": round(rc, 4), "modes": c, "box_length": round(L, 4), "steps_before": steps, "repeats": repeats,
             "step_batch": step_batch, "current_accumulate_ms": spread(t_cur[c]), "rhok_accumulate_ms": spread(t_rhok[c]),
             "current_over_rhok": round(min(t_cur[c]) / min(t_rhok[c]), 3), "md_step_ms": round(step, 5),
             "current_over_step": round(min(t_cur[c]) / step, 4)} for c in counts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "current_resident_rate.txt")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--step-batch", type=int, default=20)
    ap.add_argument("--modes", type=int, nargs="*", default=[64, 1024, 4096])
    ap.add_argument("n", type=int, nargs="*", default=[4096, 65536, 262144])
    a = ap.parse_args()
    a.out.parent.mkdir(parents=True, exist_ok=True)
    with open(a.out, "w") as f:
        for n in a.n:
            for rc in (None, 2.5):
                for line in measure(n, rc, a.modes, a.steps, a.repeats, a.step_batch):
                    text = json.dumps(line)
                    print(text, flush=True)
                    f.write(text + "\n")
                    f.flush()


if __name__ == "__main__":
    main()
