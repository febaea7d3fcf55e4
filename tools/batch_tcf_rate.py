#!/usr/bin/env python3
"""Cost of the batch engine's on-device MSD / VACF (BatchEngine.tcf_*, ljmd_batch_tcf_*), measured in one process on one
card.  One JSON line per (n, B), also written to profiles/batch_tcf_rate.txt (--out PATH for another file):

  (a) stepping with the feature inside: steps(1000, sample_every=100) on one handle, first with it off, then with
      tcf_configure(50, 1, every=100) -- ten snapshots per call, and from the sixth call on every snapshot meets the full
      50 live origins (the warm-up fills the ring: five calls)
        off_replica_steps_per_s / tcf_replica_steps_per_s   B * steps / wall time of the call
        ratio                      tcf / off: the price of the feature at one snapshot per 100 steps
        off_kernel_ms / tcf_kernel_ms, off_launches / tcf_launches   ljmd_batch_profile_read of the best call
        tcf_pass_kernel_ms         (tcf_kernel_ms - off_kernel_ms) / 10: one snapshot against 50 origins, all replicas
        tcf_pass_in_steps          tcf_pass_kernel_ms / (off_kernel_ms / steps): that pass in force steps
        ring_read_GBps             bytes of the 50 ring slots of all replicas / tcf_pass_kernel_ms
  (b) the same ten snapshots by the route without the feature: ten get_state calls of all twelve planes (timed in
      full), the planes split per replica, and ljmd_time_origin_average (analysis.time_origin_average_gpu) for MSD and
      for VACF per replica on its ten-snapshot trajectory -- timed on the first 64 replicas and SCALED by B / 64
      (host_route10_ms_scaled, of which get_state10_ms); on_device10_ms is the wall time of the call of (a) minus that
      of the call with the feature off, plus one tcf_read.  A ten-snapshot trajectory has lags up to 9 only, while the
      device meets 50 origins per snapshot: the host route does less work, so speedup_vs_host_route is a lower bound.

Usage: batch_tcf_rate.py [--out PATH] [n:B[:steps] ...]   Default: 108:4096 500:1024, 1000 steps per call.
Each figure is the best of three calls after the warm-up.  Measurement tool."""
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
MAX_LAG = 50
SCALED_FROM = 64


def best_steps(eng, B, steps, warmup):
    for _ in range(warmup):
        eng.steps(steps, SAMPLE)
    best, prof, wall = 0.0, None, None
    for _ in range(3):
        t0 = time.perf_counter()
        e, k, _, _ = eng.steps(steps, SAMPLE)
        dt = time.perf_counter() - t0
        if B * steps / dt > best:
            best, prof, wall = B * steps / dt, eng.profile_read(), dt
    assert np.all(np.isfinite(e)) and np.all(np.isfinite(k))
    return best, prof, wall


def measure(n, B, steps):
    p, _, _ = synthetic.make_config(n)
    cfg = [synthetic.make_config(n, seed=1000 + b) for b in range(min(B, 64))]
    r = np.stack([cfg[b % len(cfg)][1] for b in range(B)])               # [B, 3, n]
    v = np.stack([cfg[b % len(cfg)][2] for b in range(B)])
    snapshots = steps // SAMPLE
    with BatchEngine(p, B) as eng:
        eng.set_state(r[:, 0], r[:, 1], r[:, 2], v[:, 0], v[:, 1], v[:, 2])
        eng.compute_forces()
        off, off_prof, off_wall = best_steps(eng, B, steps, 1)
        eng.tcf_configure(MAX_LAG, 1, every=SAMPLE)
        on, on_prof, on_wall = best_steps(eng, B, steps, -(-MAX_LAG // snapshots))
        t0 = time.perf_counter()
        msd, vacf, counts, count = eng.tcf_read()
        read_ms = 1e3 * (time.perf_counter() - t0)
        assert count == (3 + -(-MAX_LAG // snapshots)) * snapshots and counts[MAX_LAG] > 0
        assert np.all(np.isfinite(msd)) and msd[:, MAX_LAG].min() > 0.0 and np.all(np.isfinite(vacf))
        pass_ms = (on_prof["kernel_ms"] - off_prof["kernel_ms"]) / snapshots
        device_ms = 1e3 * (on_wall - off_wall) + read_ms

        # (b) the route without the feature: download every sampling instant, then one stateless call per replica and kind
        eng.tcf_configure(0)
        m = min(B, SCALED_FROM)
        get_ms = avg_ms = float("inf")
        for _ in range(3):
            t0 = time.perf_counter()
            traj = []
            for _ in range(snapshots):
                st = eng.get_state(("r", "ru", "v", "a"))                # all twelve planes, as a segmented run reads
                traj.append((st["ru"], st["v"]))
            t1 = time.perf_counter()
            for b in range(m):
                ru = [np.stack([s[0][ax][b] for s in traj]) for ax in range(3)]      # [snapshots, n] per axis
                vv = [np.stack([s[1][ax][b] for s in traj]) for ax in range(3)]
                analysis.time_origin_average_gpu(0, *ru, max_lag=MAX_LAG)
                analysis.time_origin_average_gpu(1, *vv, max_lag=MAX_LAG)
            t2 = time.perf_counter()
            get_ms, avg_ms = min(get_ms, 1e3 * (t1 - t0)), min(avg_ms, 1e3 * (t2 - t1))
    ring_bytes = MAX_LAG * 6 * 8 * n * B
    return {"n": n, "replicas": B, "steps_per_call": steps, "sample_every": SAMPLE, "tcf_every": SAMPLE,
            "max_lag": MAX_LAG, "origin_stride": 1,
            "off_replica_steps_per_s": round(off, 1), "tcf_replica_steps_per_s": round(on, 1),
            "ratio": round(on / off, 4),
            "off_kernel_ms": round(off_prof["kernel_ms"], 3), "tcf_kernel_ms": round(on_prof["kernel_ms"], 3),
            "off_launches": off_prof["launches"], "tcf_launches": on_prof["launches"],
            "tcf_pass_kernel_ms": round(pass_ms, 4),
            "tcf_pass_in_steps": round(pass_ms / (off_prof["kernel_ms"] / steps), 2),
            "ring_read_GBps": round(ring_bytes / (pass_ms * 1e-3) / 1e9, 1) if pass_ms > 0 else None,
            "on_device10_ms": round(device_ms, 3), "tcf_read_ms": round(read_ms, 3),
            "host_route10_ms_scaled": round(get_ms + avg_ms * B / m, 1),
            "get_state10_ms": round(get_ms, 1), "host_route_scaled_from_replicas": m,
            "speedup_vs_host_route": round((get_ms + avg_ms * B / m) / device_ms, 1) if device_ms > 0 else None}


def main(argv):
    out = ROOT / "profiles" / "batch_tcf_rate.txt"
    if argv[:1] == ["--out"]:
        out, argv = Path(argv[1]), argv[2:]
    cases = [tuple(map(int, a.split(":"))) for a in argv] or [(108, 4096), (500, 1024)]
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
