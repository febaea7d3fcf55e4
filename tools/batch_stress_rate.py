#!/usr/bin/env python3
"""Cost of the batch engine's on-device pressure tensor (BatchEngine.stress_*, ljmd_batch_stress_*), measured in one
process on one card.  One JSON line per (n, B, rc), also written to profiles/batch_stress_rate.txt (--out PATH for another
file).  Every figure is the minimum of 5 repeats, with the spread (max - min) / min of the five beside it:

  accumulate_ms              one stress_accumulate of all B replicas, from the call to the device being idle again
                             (a read of the snapshot count, which waits); the series is reset in between
  off_replica_steps_per_s / stress_replica_steps_per_s
                             B * steps / wall time of steps(steps, observables=False), with the feature off and with
                             stress_configure(steps / 10, every=10); the two alternate, off first
  ratio                      stress / off: the price of one snapshot per 10 steps
  accumulate_in_steps        accumulate_ms / (wall time of one step with the feature off)
  the route it replaces, in the same process:
  get_state_ms               get_state(("r", "v")) of all replicas: the transfer a host evaluation starts with
  numpy_one_replica_ms       tests/stress_model.py's pair loop for ONE replica
  host_route_ms_scaled       get_state_ms + B * numpy_one_replica_ms -- SCALED from one replica, not measured at B

Usage: batch_stress_rate.py [--out PATH] [n:B:steps[:rc] ...]   Default: 108:4096:1000 500:1024:200 4000:256:20 with the
cutoff of synthetic.make_config (rc = 0.49 L: nearly half of all pairs lie inside it), then the same three with rc = 2.5
(1 to 12 % of the pairs inside), the cutoff the cost estimate of DESIGN.md 3.10 was made for.
Measurement tool."""
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import ljmd_amd  # noqa: E402,F401
import stress_model  # noqa: E402
from ljmd_amd import BatchEngine, md_types, synthetic  # noqa: E402

REPEATS = 5
EVERY = 10


def low(xs):
    """-> (minimum, spread of the repeats relative to it)"""
    return min(xs), (max(xs) - min(xs)) / min(xs)


def timed(call):
    t0 = time.perf_counter()
    call()
    return time.perf_counter() - t0


def measure(n, B, steps, rc=None):
    p, _, _ = synthetic.make_config(n)
    if rc is not None:
        p = md_types.init_params(n, p.box_length, p.dt, rc)
    cfg = [synthetic.make_config(n, seed=1000 + b) for b in range(min(B, 64))]
    r = np.stack([cfg[b % len(cfg)][1] for b in range(B)])               # [B, 3, n]
    v = np.stack([cfg[b % len(cfg)][2] for b in range(B)])
    snapshots = steps // EVERY
    with BatchEngine(p, B) as eng:
        eng.set_state(r[:, 0], r[:, 1], r[:, 2], v[:, 0], v[:, 1], v[:, 2])
        eng.compute_forces()
        eng.steps(steps, observables=False)                              # warm-up

        eng.stress_configure(2)

        def one_accumulate():
            eng.stress_accumulate()
            eng._stress_rows("batch_stress_rate")                        # waits for the device

        one_accumulate()
        acc = []
        for _ in range(REPEATS):
            eng.stress_reset()
            eng._stress_rows("batch_stress_rate")
            acc.append(timed(one_accumulate))
        words = eng.stress_read_exact(raw=True)
        assert words.shape == (1, B, 12, 3) and words[0, :, 0].any()

        off, on = [], []
        for _ in range(REPEATS):
            eng.stress_configure(0)
            off.append(timed(lambda: eng.steps(steps, observables=False)))
            eng.stress_configure(snapshots, every=EVERY)
            on.append(timed(lambda: eng.steps(steps, observables=False)))
            assert eng._stress_rows("batch_stress_rate") == snapshots
        on_prof = eng.profile_read()
        eng.stress_configure(0)

        get = []
        for _ in range(REPEATS):
            get.append(timed(lambda: eng.get_state(("r", "v"))))
        st = eng.get_state(("r", "v"))
        r0 = np.stack([st["r"][ax][0] for ax in range(3)])
        v0 = np.stack([st["v"][ax][0] for ax in range(3)])
        host = [timed(lambda: stress_model.words(r0, v0, p.box_length, p.rc)) for _ in range(REPEATS if n <= 1000 else 2)]

    (acc_s, acc_sp), (off_s, off_sp), (on_s, on_sp), (get_s, get_sp) = low(acc), low(off), low(on), low(get)
    host_s, _ = low(host)
    return {"n": n, "replicas": B, "rc": round(p.rc, 6), "rc_over_L": round(p.rc / p.box_length, 4),
            "steps_per_call": steps, "stress_every": EVERY, "repeats": REPEATS,
            "accumulate_ms": round(1e3 * acc_s, 4), "accumulate_spread": round(acc_sp, 3),
            "off_replica_steps_per_s": round(B * steps / off_s, 1), "off_spread": round(off_sp, 3),
            "stress_replica_steps_per_s": round(B * steps / on_s, 1), "stress_spread": round(on_sp, 3),
            "ratio": round(off_s / on_s, 4),
            "stress_launches": on_prof["launches"], "stress_kernel_ms": round(on_prof["kernel_ms"], 3),
            "accumulate_in_steps": round(acc_s / (off_s / steps), 2),
            "get_state_ms": round(1e3 * get_s, 3), "get_state_spread": round(get_sp, 3),
            "numpy_one_replica_ms": round(1e3 * host_s, 2),
            "host_route_ms_scaled": round(1e3 * (get_s + B * host_s), 1), "host_route_scaled_from_replicas": 1,
            "speedup_vs_host_route_scaled": round((get_s + B * host_s) / acc_s, 1)}


def main(argv):
    out = ROOT / "profiles" / "batch_stress_rate.txt"
    if argv[:1] == ["--out"]:
        out, argv = Path(argv[1]), argv[2:]
    sizes = [(108, 4096, 1000), (500, 1024, 200), (4000, 256, 20)]
    cases = [tuple(float(x) if k == 3 else int(x) for k, x in enumerate(a.split(":"))) for a in argv] or \
        sizes + [c + (2.5,) for c in sizes]
    out.parent.mkdir(parents=True, exist_ok=True)
    with open(out, "w") as f:
        for case in cases:
            line = json.dumps(measure(*case))
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()


if __name__ == "__main__":
    main(sys.argv[1:])
