#!/usr/bin/env python3
"""Cost of the engine's resident pressure tensor (Engine.stress_*, ljmd_stress_*), measured in one process on one card.
One JSON line per (system size, cutoff), also written to profiles/stress_resident_rate.txt (--out PATH for another file).

The system is the bench workload's recipe (synthetic.make_config: rho = 0.8, jittered lattice) with rc = 0.49 L and with
rc = 2.5, advanced --steps steps (default 300) so that the tiles are between two re-sorts.  Then, alternating, --repeats
times (default 5) after one warm-up round, each figure reported as its minimum and its spread (max - min):

  accumulate_ms       ljmd_stress_profile_read's kernel time (HIP events around the four launches) of one
                      stress_accumulate, and visited_fraction = tile pairs evaluated / considered
  md_step_ms          one MD step of the same handle: wall time of --step-batch (default 100) enqueued steps / that many
  segment_plain_ms    wall time of one enqueued --step-batch segment, collected
  segment_stress_ms   the same with one stress_accumulate enqueued behind the segment, read with the records
  get_state_ms        the only route without the feature, its device half: one get_state of r and v per instant

accumulate_over_step = accumulate_ms / md_step_ms.  host_pair_loop_ms is the rest of that route, a numpy minimum-image
pass over all ordered pairs timed ONCE at N = 4096 with the line's cutoff (0.49 L or 2.5) and SCALED by the number of pairs to
the line's n (stated as scaled: it is not measured at that size).

Usage: stress_resident_rate.py [--out PATH] [--steps K] [--repeats R] [--step-batch S] [n ...]
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
from ljmd_amd import Engine, md_types, synthetic  # noqa: E402


def spread(xs):
    return {"min": round(min(xs), 4), "spread": round(max(xs) - min(xs), 4)}


def host_pair_loop_ms(r, v, L, rc):
    """the six sums in doubles over all ordered pairs, rows in chunks of 256: what a host route has to do per instant"""
    t0 = time.perf_counter()
    n = r.shape[1]
    acc = np.zeros(6)
    for i0 in range(0, n, 256):
        d = [r[k, i0:i0 + 256, None] - r[k][None, :] for k in range(3)]
        d = [x - L * np.round(x / L) for x in d]
        r2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
        inside = (r2 < rc * rc) & (r2 > 0.0)
        u = 1.0 / r2[inside]
        m = (2.0 * u ** 6 - u ** 3) * u
        dd = [x[inside] for x in d]
        for c, (a, b) in enumerate(((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))):
            acc[c] += np.sum(m * dd[a] * dd[b])
    acc[:3] += np.sum(v * v, axis=1)
    return 1e3 * (time.perf_counter() - t0)


def measure(n, rc, steps, repeats, step_batch, host4096_ms):
    p, r, v = synthetic.make_config(n)
    L = p.box_length
    rc = 0.49 * L if rc is None else rc
    p = md_types.init_params(n, L, p.dt, rc)
    with Engine(p) as eng:
        eng.set_state(r[0], r[1], r[2], v[0], v[1], v[2])
        eng.compute_forces()
        eng.advance(steps)
        eng.stress_configure(4 * (repeats + 1))
        t_acc, t_plain, t_stress, t_get = [], [], [], []
        frac = None
        for rep in range(repeats + 1):                       # round 0 warms every path up
            eng.stress_accumulate()
            prof = eng.stress_profile()                      # waits for the device
            frac = prof["tile_pairs_visited"] / prof["tile_pairs_total"]
            t0 = time.perf_counter()
            eng.enqueue_steps(step_batch)
            eng.collect_steps(step_batch)
            t1 = time.perf_counter()
            eng.enqueue_steps(step_batch)
            eng.stress_accumulate()
            eng.collect_steps(step_batch)
            eng.stress_read()
            t2 = time.perf_counter()
            eng.get_state(("r", "v"))
            t3 = time.perf_counter()
            if rep:
                t_acc.append(prof["kernel_ms"])
                t_plain.append(1e3 * (t1 - t0))
                t_stress.append(1e3 * (t2 - t1))
                t_get.append(1e3 * (t3 - t2))
    step = min(t_plain) / step_batch
    return {"n": n, "box_length": round(L, 4), "rc": round(rc, 4), "steps_before": steps, "repeats": repeats,
            "step_batch": step_batch,
            "accumulate_ms": spread(t_acc), "visited_fraction": round(frac, 4),
            "md_step_ms": round(step, 5), "accumulate_over_step": round(min(t_acc) / step, 3),
            "segment_plain_ms": spread(t_plain), "segment_stress_ms": spread(t_stress),
            "steps_per_s_plain": round(1e3 * step_batch / min(t_plain), 2),
            "steps_per_s_stress": round(1e3 * step_batch / min(t_stress), 2),
            "get_state_ms": spread(t_get),
            "host_pair_loop_ms_scaled_from_n4096": round(host4096_ms * (n * (n - 1.0)) / (4096 * 4095.0), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "stress_resident_rate.txt")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--step-batch", type=int, default=100)
    ap.add_argument("n", type=int, nargs="*", default=[4096, 65536, 262144])
    a = ap.parse_args()
    a.out.parent.mkdir(parents=True, exist_ok=True)
    p0, r0, v0 = synthetic.make_config(4096)
    host = {None: host_pair_loop_ms(r0, v0, p0.box_length, 0.49 * p0.box_length),
            2.5: host_pair_loop_ms(r0, v0, p0.box_length, 2.5)}
    with open(a.out, "w") as f:
        for n in a.n:
            for rc in (None, 2.5):
                line = json.dumps(measure(n, rc, a.steps, a.repeats, a.step_batch, host[rc]))
                print(line, flush=True)
                f.write(line + "\n")
                f.flush()


if __name__ == "__main__":
    main()
