#!/usr/bin/env python3
"""Cost of the engine's resident MSD / VACF (Engine.tcf_*, ljmd_tcf_*), measured in one process on one card.  One JSON
line per (system size, live origins), also written to profiles/tcf_resident_rate.txt (--out PATH for another file).

The system is the bench workload's recipe (synthetic.make_config: rho = 0.8, rc = 0.49 L, jittered lattice), advanced
--steps steps (default 100).  For `live` live origins the feature is configured with max_lag = 2 live - 1 and origin
stride 2 (`live` ring slots), and 2 live snapshots are taken: from then on every snapshot with an odd number meets
exactly `live` origins.  Then, alternating, --repeats times (default 5) after one warm-up round, each figure reported as
its minimum and its spread (max - min):

  resident_ms         ljmd_tcf_profile_read's kernel time (HIP events around the launches) of one tcf_accumulate that
                      visits `live` origins (origins_live is checked), and gbytes_per_s = 48 n_pad live / that time
  snapshot_ms         the route that exists without the feature, per sampling instant: ljmd_snapshot_begin + _end of the
                      full state to the host (host clock)
  origin_average_ms   ... and, once per run, one ljmd_time_origin_average per kind (MSD, then VACF; host clock around the
                      blocking call: upload, kernel, download) over live + 1 collected snapshots with max_lag = live.
                      null when the collected snapshots would exceed --host-bytes (default 8e9) of host memory.

resident_run_ms = (live + 1) resident_ms and parent_run_ms = (live + 1) snapshot_ms + the two origin averages compare
the two routes over a run of live + 1 sampling instants (the resident figure an upper bound: the first `live` snapshots
meet fewer origins).  No pass mark.

Usage: tcf_resident_rate.py [--out PATH] [--steps K] [--repeats R] [--live 16 128 512] [n ...]
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
from ljmd_amd import Engine, analysis, synthetic  # noqa: E402


def spread(xs):
    return {"min": round(min(xs), 4), "spread": round(max(xs) - min(xs), 4)}


def resident_once(eng, live):
    """two snapshots; -> kernel ms of the odd-numbered one, which meets `live` origins"""
    eng.tcf_accumulate()                                     # even number: live - 1 origins, stored
    eng.tcf_accumulate()
    prof = eng.tcf_profile()                                 # waits for the device
    assert prof["origins_live"] == live, prof
    return prof["kernel_ms"]


def measure(n, live, steps, repeats, host_bytes):
    p, r, v = synthetic.make_config(n)
    n_pad = (n + 1023) // 1024 * 1024
    with Engine(p) as eng:
        eng.set_state(r[0], r[1], r[2], v[0], v[1], v[2])
        eng.compute_forces()
        eng.advance(steps)
        eng.tcf_configure(2 * live - 1, 2)
        for _ in range(2 * live):
            eng.tcf_accumulate()
        t_res, t_snap = [], []
        for rep in range(repeats + 1):                       # round 0 warms both paths up
            a = resident_once(eng, live)
            t0 = time.perf_counter()
            eng.snapshot_begin()
            snap = eng.snapshot_end()
            t1 = time.perf_counter()
            if rep:
                t_res.append(a)
                t_snap.append(1e3 * (t1 - t0))
        eng.tcf_configure(0)
        # the parent route's analysis: live + 1 collected snapshots (the same one repeated: the time does not depend on
        # the values), one blocking call per kind
        t_avg = None
        if 2 * 3 * (live + 1) * n * 8 <= host_bytes:
            ru = [np.ascontiguousarray(np.broadcast_to(snap["ru"][ax], (live + 1, n))) for ax in range(3)]
            vv = [np.ascontiguousarray(np.broadcast_to(snap["v"][ax], (live + 1, n))) for ax in range(3)]
            t_avg = []
            for rep in range(repeats + 1):
                t0 = time.perf_counter()
                analysis.time_origin_average_gpu(0, *ru, max_lag=live)
                analysis.time_origin_average_gpu(1, *vv, max_lag=live)
                t1 = time.perf_counter()
                if rep:
                    t_avg.append(1e3 * (t1 - t0))
    res = min(t_res)
    out = {"n": n, "live_origins": live, "steps_before": steps, "repeats": repeats,
           "resident_ms": spread(t_res), "gbytes_per_s": round(48.0 * n_pad * live / (res * 1e-3) / 1e9, 1),
           "snapshot_ms": spread(t_snap), "origin_average_ms": spread(t_avg) if t_avg else None,
           "resident_run_ms": round((live + 1) * res, 3)}
    if t_avg:
        out["parent_run_ms"] = round((live + 1) * min(t_snap) + min(t_avg), 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "tcf_resident_rate.txt")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--live", type=int, nargs="+", default=[16, 128, 512])
    ap.add_argument("--host-bytes", type=float, default=8e9)
    ap.add_argument("n", type=int, nargs="*", default=[4096, 65536, 262144])
    a = ap.parse_args()
    a.out.parent.mkdir(parents=True, exist_ok=True)
    with open(a.out, "w") as f:
        for n in a.n:
            for live in a.live:
                line = json.dumps(measure(n, live, a.steps, a.repeats, a.host_bytes))
                print(line, flush=True)
                f.write(line + "\n")
                f.flush()


if __name__ == "__main__":
    main()
