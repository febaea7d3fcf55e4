#!/usr/bin/env python3
"""Cost of the batch engine's on-device heat flux (BatchEngine.heatflux_*, ljmd_batch_heatflux_*), measured in one process
on one card.  One JSON line per (n, B, rc), also written to profiles/batch_heatflux_rate.txt (--out PATH for another
file).  Every figure is the minimum of 5 repeats, with the spread (max - min) / min of the five beside it:

  accumulate_ms              one heatflux_accumulate of all B replicas, from the call to the device being idle again
                             (a read of the snapshot count, which waits); the series is reset in between
  stress_accumulate_ms       the same of stress_accumulate on the same handle; the two alternate, the heat flux first
  accumulate_in_stress       accumulate_ms / stress_accumulate_ms
  off_replica_steps_per_s / heatflux_replica_steps_per_s
                             B * steps / wall time of steps(steps, observables=False), with the feature off and with
                             heatflux_configure(steps / 10, every=10); the two alternate, off first
  ratio                      heatflux / off: the price of one snapshot per 10 steps
  accumulate_in_steps        accumulate_ms / (wall time of one step with the feature off)
  lds_chunks                 column chunks of the kernel class (csrc/ljmd_batch_heatflux.hip): 2 above n = 2048, else 1

Usage: batch_heatflux_rate.py [--out PATH] [n:B:steps[:rc] ...]   Default: 108:4096:1000 500:1024:200 4000:256:20 with the
cutoff of synthetic.make_config (rc = 0.49 L: nearly half of all pairs lie inside it), then the same three with rc = 2.5.
Measurement tool."""
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import ljmd_amd  # noqa: E402,F401
from ljmd_amd import BatchEngine, md_types, synthetic  # noqa: E402

REPEATS = 5
EVERY = 10
WHO = "batch_heatflux_rate"


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

        eng.heatflux_configure(2)
        eng.stress_configure(2)

        def one_heatflux():
            eng.heatflux_accumulate()
            eng._heatflux_rows(WHO)                                      # waits for the device

        def one_stress():
            eng.stress_accumulate()
            eng._stress_rows(WHO)

        one_heatflux()
        one_stress()
        acc, sacc = [], []
        for _ in range(REPEATS):
            eng.heatflux_reset()
            eng.stress_reset()
            eng._heatflux_rows(WHO)
            acc.append(timed(one_heatflux))
            sacc.append(timed(one_stress))
        words = eng.heatflux_read_exact(raw=True)
        assert words.shape == (1, B, 9, 3) and words[0, :, 0].any()
        eng.stress_configure(0)

        off, on = [], []
        for _ in range(REPEATS):
            eng.heatflux_configure(0)
            off.append(timed(lambda: eng.steps(steps, observables=False)))
            eng.heatflux_configure(snapshots, every=EVERY)
            on.append(timed(lambda: eng.steps(steps, observables=False)))
            assert eng._heatflux_rows(WHO) == snapshots
        on_prof = eng.profile_read()
        eng.heatflux_configure(0)

    (acc_s, acc_sp), (sacc_s, sacc_sp), (off_s, off_sp), (on_s, on_sp) = low(acc), low(sacc), low(off), low(on)
    return {"n": n, "replicas": B, "rc": round(p.rc, 6), "rc_over_L": round(p.rc / p.box_length, 4),
            "lds_chunks": 2 if n > 2048 else 1, "steps_per_call": steps, "heatflux_every": EVERY, "repeats": REPEATS,
            "accumulate_ms": round(1e3 * acc_s, 4), "accumulate_spread": round(acc_sp, 3),
            "stress_accumulate_ms": round(1e3 * sacc_s, 4), "stress_accumulate_spread": round(sacc_sp, 3),
            "accumulate_in_stress": round(acc_s / sacc_s, 3),
            "off_replica_steps_per_s": round(B * steps / off_s, 1), "off_spread": round(off_sp, 3),
            "heatflux_replica_steps_per_s": round(B * steps / on_s, 1), "heatflux_spread": round(on_sp, 3),
            "ratio": round(off_s / on_s, 4),
            "heatflux_launches": on_prof["launches"], "heatflux_kernel_ms": round(on_prof["kernel_ms"], 3),
            "accumulate_in_steps": round(acc_s / (off_s / steps), 2)}


def main(argv):
    out = ROOT / "profiles" / "batch_heatflux_rate.txt"
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
