#!/usr/bin/env python3
"""Step rate of the batch engine in the reproducible mode (BatchEngine(precision_mode=2), ljmd_batch_set_precision)
against the two things it stands beside, measured in the same process on the same card.  One JSON line per (n, B):

  reproducible_replica_steps_per_s   B * steps / wall time of ljmd_batch_steps(steps, sample_every = 100), reproducible
  fp64_replica_steps_per_s           the same call on an fp64 batch handle
  single_reproducible_steps_per_s    one Engine(precision_mode=2): enqueue_steps(100, sampled=True) + collect_steps, the
                                     production loop's form -- the only way to these bits without the batch mode
  ratio_vs_single                    reproducible_replica_steps_per_s / single_reproducible_steps_per_s: above 1, the
                                     batch beats running the same replicas one after another on the single engine
  ratio_vs_fp64                      reproducible_replica_steps_per_s / fp64_replica_steps_per_s: the price of the mode
  kernel_ms_per_launch               HIP-event time of the reproducible batch kernels of one call / launches of that call
  steps_per_launch                   steps_per_call / launches_per_call: the mean when the call's last launch is short

Usage: batch_reproducible_rate.py [n:B[:steps] ...]   Default: 108:4096 500:1024 4000:256 over 1000 / 1000 / 100 steps,
the rates; then calls that are a whole number of full launches of the library's launch bounds (csrc/ljmd_batch.cpp), so
that kernel_ms_per_launch is the time of a full launch: 108:4096:1500 (20 x 75 steps) and 500:1024:700 (50 x 14), and
B = 1 at n = 108, 500, 4000 (3 x 333, 6 x 56, 10 x 1: a workgroup alone on its CU, where latency sets the launch
length).  At 4000:256 a launch is one step, so the first run of it is one of whole launches already.
Each figure is the best of three calls after a warm-up call.  Measurement tool."""
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import ljmd_amd  # noqa: E402,F401
from ljmd_amd import BatchEngine, Engine, _lib, synthetic  # noqa: E402

SAMPLE = 100
MODE = _lib.PRECISION_FP64_REPRODUCIBLE


def single_rate(n: int, segments: int) -> float:
    p, r, v = synthetic.make_config(n)
    with Engine(p, precision_mode=MODE) as eng:
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


def batch_rate(n: int, B: int, steps: int, mode: int):
    p, _, _ = synthetic.make_config(n)
    cfg = [synthetic.make_config(n, seed=1000 + b) for b in range(min(B, 64))]
    r = np.stack([cfg[b % len(cfg)][1] for b in range(B)])           # [B, 3, n]
    v = np.stack([cfg[b % len(cfg)][2] for b in range(B)])
    every = SAMPLE if steps % SAMPLE == 0 else steps
    with BatchEngine(p, B, precision_mode=mode) as eng:
        eng.set_state(r[:, 0], r[:, 1], r[:, 2], v[:, 0], v[:, 1], v[:, 2])
        eng.compute_forces()
        eng.steps(steps, every)                                          # warm-up
        best, prof = 0.0, None
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
        [(108, 4096), (500, 1024), (4000, 256), (108, 4096, 1500), (500, 1024, 700),
         (108, 1, 999), (500, 1, 336), (4000, 1, 10)]
    for case in cases:
        n, B = case[:2]
        steps = case[2] if len(case) > 2 else 1000 if n <= 1000 else 100
        every = SAMPLE if steps % SAMPLE == 0 else steps
        single = single_rate(n, segments=20 if n <= 1000 else 5)
        fp64, _ = batch_rate(n, B, steps, _lib.PRECISION_FP64)
        rate, prof = batch_rate(n, B, steps, MODE)
        print(json.dumps({"n": n, "replicas": B, "steps_per_call": steps, "sample_every": every,
                          "reproducible_replica_steps_per_s": round(rate, 1),
                          "fp64_replica_steps_per_s": round(fp64, 1),
                          "single_reproducible_steps_per_s": round(single, 1),
                          "ratio_vs_single": round(rate / single, 2), "ratio_vs_fp64": round(rate / fp64, 3),
                          "launches_per_call": prof["launches"],
                          "steps_per_launch": round(steps / max(prof["launches"], 1), 2),
                          "kernel_ms_per_launch": round(prof["kernel_ms"] / max(prof["launches"], 1), 3),
                          "kernel_ms_per_call": round(prof["kernel_ms"], 3)}), flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
