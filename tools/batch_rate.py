#!/usr/bin/env python3
"""Aggregate step rate of the batch engine (BatchEngine, ljmd_batch_*) against the single engine at the same n,
measured in the same process on the same card.  One JSON line per (n, B):

  batch_replica_steps_per_s   B * steps / wall time of ljmd_batch_steps(steps, sample_every = 100)
  single_steps_per_s          one Engine: enqueue_steps(100, sampled=True) + collect_steps, the production loop's form
  ratio                       batch_replica_steps_per_s / single_steps_per_s
  kernel_ms_per_launch        HIP-event time of the batch kernels of one call / launches of that call

Usage: batch_rate.py [n:B[:steps] ...]   (default 108:4096 500:1024 4000:256, then B = 1 at n = 108, 500, 4000 with the
steps of exactly one full launch: a workgroup alone on its CU, where the launch length is set by latency).
Measurement tool."""
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import ljmd_amd  # noqa: E402,F401
from ljmd_amd import BatchEngine, Engine, synthetic  # noqa: E402

SAMPLE = 100


def single_rate(n: int, segments: int) -> float:
    p, r, v = synthetic.make_config(n)
    with Engine(p) as eng:
        eng.set_state(r[0], r[1], r[2], v[0], v[1], v[2])
        eng.compute_forces()
        eng.enqueue_steps(SAMPLE, sampled=True)
        eng.collect_steps(SAMPLE)
        best = 0.0
        for _ in range(3):
            eng.synchronize()
            t0 = time.perf_counter()
            for _ in range(segments):
                eng.enqueue_steps(SAMPLE, sampled=True)
                eng.collect_steps(SAMPLE)
            best = max(best, segments * SAMPLE / (time.perf_counter() - t0))
    return best


def batch_rate(n: int, B: int, steps: int):
    p, _, _ = synthetic.make_config(n)
    cfg = [synthetic.make_config(n, seed=1000 + b) for b in range(min(B, 64))]
    r = np.stack([cfg[b % len(cfg)][1] for b in range(B)])           # [B, 3, n]
    v = np.stack([cfg[b % len(cfg)][2] for b in range(B)])
    with BatchEngine(p, B) as eng:
        eng.set_state(r[:, 0], r[:, 1], r[:, 2], v[:, 0], v[:, 1], v[:, 2])
        eng.compute_forces()
        eng.steps(SAMPLE, SAMPLE)                                        # warm-up
        best, prof = 0.0, None
        every = SAMPLE if steps % SAMPLE == 0 else steps
        for _ in range(3):
            t0 = time.perf_counter()
            e, k, d, dd = eng.steps(steps, every)
            dt = time.perf_counter() - t0
            if B * steps / dt > best:
                best, prof = B * steps / dt, eng.profile_read()
        assert np.all(np.isfinite(e)) and np.all(np.isfinite(k))
    return best, prof


def main(argv):
    cases = [tuple(map(int, a.split(":"))) for a in argv] or \
        [(108, 4096), (500, 1024), (4000, 256), (108, 1, 1851), (500, 1, 312), (4000, 1, 4)]
    for case in cases:
        n, B = case[:2]
        single = single_rate(n, segments=20 if n <= 1000 else 5)
        steps = case[2] if len(case) > 2 else 1000 if n <= 1000 else 100
        rate, prof = batch_rate(n, B, steps)
        every = SAMPLE if steps % SAMPLE == 0 else steps
        print(json.dumps({"n": n, "replicas": B, "steps_per_call": steps, "sample_every": every,
                          "batch_replica_steps_per_s": round(rate, 1), "single_steps_per_s": round(single, 1),
                          "ratio": round(rate / single, 2), "launches_per_call": prof["launches"],
                          "kernel_ms_per_launch": round(prof["kernel_ms"] / max(prof["launches"], 1), 3),
                          "kernel_ms_per_call": round(prof["kernel_ms"], 3)}), flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
