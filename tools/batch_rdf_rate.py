#!/usr/bin/env python3
"""Cost of the batch engine's on-device g(r) (BatchEngine.rdf_*, ljmd_batch_rdf_*), measured in one process on one card.
One JSON line per (n, B), also written to profiles/batch_rdf_rate.txt (--out PATH for another file):

  (a) stepping with g(r) inside: steps(1000, sample_every=100) on one handle, first with g(r) off, then with
      rdf_configure(200, every=100) -- ten snapshots per call
        off_replica_steps_per_s / rdf_replica_steps_per_s   B * steps / wall time of the call
        ratio                      rdf / off: the price of the feature at one snapshot per 100 steps
        off_kernel_ms / rdf_kernel_ms, off_launches / rdf_launches   ljmd_batch_profile_read of the best call
        rdf_pass_kernel_ms         (rdf_kernel_ms - off_kernel_ms) / 10: one g(r) pass over all replicas
        rdf_pass_in_steps          rdf_pass_kernel_ms / (off_kernel_ms / steps): that pass in force steps
  (b) ten rdf_accumulate calls and one rdf_read, wall time (accumulate10_ms), beside the route without the feature for
      the same ten snapshots: get_state of all replicas, then one ljmd_rdf_histogram call per replica.  The histogram
      calls are timed on the first 64 replicas of one snapshot and SCALED by B / 64 and by ten; get_state is timed in
      full (host_route10_ms_scaled, of which get_state10_ms).  The two histograms of those 64 replicas must be equal.

Usage: batch_rdf_rate.py [--out PATH] [n:B[:steps] ...]   Default: 108:4096 500:1024 4000:256, 1000 steps per call.
Each figure is the best of three calls after a warm-up call.  Measurement tool."""
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import ljmd_amd  # noqa: E402,F401
from ljmd_amd import BatchEngine, analysis, synthetic  # noqa: E402

SAMPLE = 100
NBINS = 200
SCALED_FROM = 64


def best_steps(eng, B, steps):
    eng.steps(steps, SAMPLE)                                             # warm-up
    best, prof = 0.0, None
    for _ in range(3):
        t0 = time.perf_counter()
        e, k, _, _ = eng.steps(steps, SAMPLE)
        dt = time.perf_counter() - t0
        if B * steps / dt > best:
            best, prof = B * steps / dt, eng.profile_read()
    assert np.all(np.isfinite(e)) and np.all(np.isfinite(k))
    return best, prof


def measure(n, B, steps):
    p, _, _ = synthetic.make_config(n)
    cfg = [synthetic.make_config(n, seed=1000 + b) for b in range(min(B, 64))]
    r = np.stack([cfg[b % len(cfg)][1] for b in range(B)])               # [B, 3, n]
    v = np.stack([cfg[b % len(cfg)][2] for b in range(B)])
    L = p.box_length
    with BatchEngine(p, B) as eng:
        eng.set_state(r[:, 0], r[:, 1], r[:, 2], v[:, 0], v[:, 1], v[:, 2])
        eng.compute_forces()
        off, off_prof = best_steps(eng, B, steps)
        eng.rdf_configure(NBINS, every=SAMPLE)
        on, on_prof = best_steps(eng, B, steps)
        hist, count = eng.rdf_read()
        assert count == 4 * (steps // SAMPLE) and hist.sum() > 0
        snapshots = steps // SAMPLE
        pass_ms = (on_prof["kernel_ms"] - off_prof["kernel_ms"]) / snapshots

        # (b) ten snapshots of the resident state: on the device ...
        eng.rdf_configure(NBINS)
        eng.rdf_accumulate()
        eng.rdf_read()                                                   # warm-up
        acc_ms = float("inf")
        for _ in range(3):
            eng.rdf_reset()
            t0 = time.perf_counter()
            for _ in range(10):
                eng.rdf_accumulate()
            hist, count = eng.rdf_read()
            acc_ms = min(acc_ms, 1e3 * (time.perf_counter() - t0))
        assert count == 10
        # ... and by download + one stateless call per replica (64 of them timed, then scaled)
        m = min(B, SCALED_FROM)
        get_ms = hist_ms = float("inf")
        for _ in range(3):
            t0 = time.perf_counter()
            x, y, z = eng.get_state(("r", "ru", "v", "a"))["r"]          # all twelve planes, as a segmented run reads
            t1 = time.perf_counter()
            host = np.zeros((m, NBINS), dtype=np.uint64)
            for b in range(m):
                analysis.rdf_histogram(x[b], y[b], z[b], L, NBINS, 0.5 * L, host[b])
            t2 = time.perf_counter()
            get_ms, hist_ms = min(get_ms, 1e3 * (t1 - t0)), min(hist_ms, 1e3 * (t2 - t1))
        assert np.array_equal(10 * host, hist[:m])
    return {"n": n, "replicas": B, "steps_per_call": steps, "sample_every": SAMPLE, "rdf_every": SAMPLE, "nbins": NBINS,
            "off_replica_steps_per_s": round(off, 1), "rdf_replica_steps_per_s": round(on, 1),
            "ratio": round(on / off, 4),
            "off_kernel_ms": round(off_prof["kernel_ms"], 3), "rdf_kernel_ms": round(on_prof["kernel_ms"], 3),
            "off_launches": off_prof["launches"], "rdf_launches": on_prof["launches"],
            "rdf_pass_kernel_ms": round(pass_ms, 4),
            "rdf_pass_in_steps": round(pass_ms / (off_prof["kernel_ms"] / steps), 2),
            "accumulate10_ms": round(acc_ms, 3),
            "host_route10_ms_scaled": round(10 * (get_ms + hist_ms * B / m), 1),
            "get_state10_ms": round(10 * get_ms, 1), "host_route_scaled_from_replicas": m,
            "speedup_vs_host_route": round(10 * (get_ms + hist_ms * B / m) / acc_ms, 1)}


def main(argv):
    out = ROOT / "profiles" / "batch_rdf_rate.txt"
    if argv[:1] == ["--out"]:
        out, argv = Path(argv[1]), argv[2:]
    cases = [tuple(map(int, a.split(":"))) for a in argv] or [(108, 4096), (500, 1024), (4000, 256)]
    out.parent.mkdir(parents=True, exist_ok=True)
    with open(out, "w") as f:
        for case in cases:
            n, B = case[:2]
            line = json.dumps(measure(n, B, case[2] if len(case) > 2 else 1000))
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()


if __name__ == "__main__":
    main(sys.argv[1:])
