#!/usr/bin/env python3
"""Cost of the engine's resident density modes (Engine.rhok_*, ljmd_rhok_*), measured in one process on one card.
One JSON line per (system size, cutoff, number of modes), also written to profiles/rhok_resident_rate.txt (--out PATH for another
file).

The system is the bench workload's recipe (synthetic.make_config: rho = 0.8, jittered lattice) with rc = 0.49 L (the
bench's cutoff) and with rc = 2.5 -- the accumulate does not depend on the cutoff, the MD step it is compared with does
-- advanced --steps steps (default 100) so that the tiles are between two re-sorts.  The mode list is random triples with
|n_a| <= 40 (the cost of a term does not depend on the mode).  Then, alternating, --repeats times (default 5) after one
warm-up round, each figure reported as its minimum and its spread (max - min):

  accumulate_ms       ljmd_rhok_profile_read's kernel time (HIP events around the two launches) of one rhok_accumulate
  md_step_ms          one MD step of the same handle: wall time of --step-batch (default 100) enqueued steps / that many
  segment_plain_ms    wall time of one enqueued --step-batch segment, collected
  segment_rhok_ms     the same with one rhok_accumulate enqueued behind the segment, read with the records
  get_state_ms        the only route without the feature, its device half: one get_state of r per instant

accumulate_over_step = accumulate_ms / md_step_ms.  host_sum_ms is the rest of that route, numpy's float sum of
exp(i k . r) over particles x modes, timed ONCE at N = 4096 with 1024 modes and SCALED by particles x modes to the line's
sizes (stated as scaled: it is not measured at that size).

Usage: rhok_resident_rate.py [--out PATH] [--steps K] [--repeats R] [--step-batch S] [--modes M ...] [n ...]
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


def host_sum_ms(r, L, modes):
    """rho_k in doubles over particles x modes, modes in chunks of 64: what a host route has to do per instant"""
    t0 = time.perf_counter()
    out = np.empty(len(modes), dtype=np.complex128)
    k = (2.0 * np.pi / L) * modes.astype(np.float64)
    for m0 in range(0, len(modes), 64):
        out[m0:m0 + 64] = np.exp(1j * (k[m0:m0 + 64] @ r)).sum(axis=1)
    return 1e3 * (time.perf_counter() - t0)


def measure(n, rc, counts, steps, repeats, step_batch, host_ms_per_term):
    p, r, v = synthetic.make_config(n)
    L = p.box_length
    rc = 0.49 * L if rc is None else rc
    p = md_types.init_params(n, L, p.dt, rc)
    lines = []
    with Engine(p) as eng:
        eng.set_state(r[0], r[1], r[2], v[0], v[1], v[2])
        eng.compute_forces()
        eng.advance(steps)
        t_plain, t_get = [], []
        t_acc = {c: [] for c in counts}
        t_rhok = {c: [] for c in counts}
        for rep in range(repeats + 1):                       # round 0 warms every path up
            t0 = time.perf_counter()
            eng.enqueue_steps(step_batch)
            eng.collect_steps(step_batch)
            t1 = time.perf_counter()
            eng.get_state(("r",))
            t2 = time.perf_counter()
            if rep:
                t_plain.append(1e3 * (t1 - t0))
                t_get.append(1e3 * (t2 - t1))
            for c in counts:
                eng.rhok_configure(mode_list(c), 2)
                eng.rhok_accumulate()
                prof = eng.rhok_profile()                    # waits for the device
                t3 = time.perf_counter()
                eng.enqueue_steps(step_batch)
                eng.rhok_accumulate()
                eng.collect_steps(step_batch)
                eng.rhok_read()
                t4 = time.perf_counter()
                if rep:
                    t_acc[c].append(prof["kernel_ms"])
                    t_rhok[c].append(1e3 * (t4 - t3))
        eng.rhok_configure(None, 0)
    step = min(t_plain) / step_batch
    for c in counts:
        lines.append({"n": n, "rc": round(rc, 4), "modes": c, "box_length": round(L, 4), "steps_before": steps, "repeats": repeats,
                      "step_batch": step_batch,
                      "accumulate_ms": spread(t_acc[c]), "md_step_ms": round(step, 5),
                      "accumulate_over_step": round(min(t_acc[c]) / step, 4),
                      "segment_plain_ms": spread(t_plain), "segment_rhok_ms": spread(t_rhok[c]),
                      "steps_per_s_plain": round(1e3 * step_batch / min(t_plain), 2),
                      "steps_per_s_rhok": round(1e3 * step_batch / min(t_rhok[c]), 2),
                      "get_state_ms": spread(t_get),
                      "host_sum_ms_scaled_from_n4096_m1024": round(host_ms_per_term * n * c, 1)})
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "rhok_resident_rate.txt")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--step-batch", type=int, default=100)
    ap.add_argument("--modes", type=int, nargs="*", default=[64, 1024, 4096])
    ap.add_argument("n", type=int, nargs="*", default=[4096, 65536, 262144])
    a = ap.parse_args()
    a.out.parent.mkdir(parents=True, exist_ok=True)
    p0, r0, _v0 = synthetic.make_config(4096)
    host = min(host_sum_ms(r0, p0.box_length, mode_list(1024)) for _ in range(3)) / (4096 * 1024)
    with open(a.out, "w") as f:
        for n in a.n:
            for rc in (None, 2.5):
                for line in measure(n, rc, a.modes, a.steps, a.repeats, a.step_batch, host):
                    text = json.dumps(line)
                    print(text, flush=True)
                    f.write(text + "\n")
                    f.flush()


if __name__ == "__main__":
    main()
