#!/usr/bin/env python3
"""Cost of the batch engine's on-device van Hove self-correlation (BatchEngine.vanhove_*, ljmd_batch_vanhove_*), measured
in one process on one card.  One JSON line per case, also written to profiles/batch_vanhove_rate.txt (--out PATH for
another file).  Every figure is the MINIMUM of 5 repeats, the repeats of the things compared ALTERNATING, and beside every
minimum stands its spread (max - min of the 5) under the same name with _spread.

  (a) one accumulate against ljmd_batch_tcf_accumulate with the same (max_lag, 1) on the same handle and state, the ring
      of either full: `origins` live origins.  Each is timed from the call to the end of a read without buffers behind it
      (which waits for the stream); the state moves two steps between the repeats.
        vanhove_accumulate_ms, tcf_accumulate_ms, ratio_vs_tcf
        ring_read_GBps            24 bytes per particle and live origin / vanhove_accumulate_ms
  (b) steps(steps_per_call, sample_every=100) with vanhove_configure(..., every=10) against the same call with the
      feature off on a second handle of the same size and starting state (switching it off on the first would empty the
      ring): replica-steps per second of wall time, and ljmd_batch_profile_read of the best call
        off_replica_steps_per_s, vanhove_replica_steps_per_s, steps_ratio, off_kernel_ms, vanhove_kernel_ms, launches
  (c) --parent-lib PATH: the off-rate of this tree's library against the parent commit's, each in child processes of its
      own that call the C ABI alone (create, set_state, compute_forces, steps): this, parent, parent again, alternating;
      the two parent series give the spread between two runs of the same code, within which this tree must agree
        off_this_steps_per_s, off_parent_steps_per_s, off_parent_again_steps_per_s
  (d) the route the feature replaces: get_state of ru per snapshot and numpy binning per live origin (differences, r2,
      sqrt, floor, bincount, sums of r2 and r4), timed on the first 64 replicas (fewer where the host's ring would pass 1 GB) and SCALED by B / that number
        host_route_ms_scaled (of which get_state_ms), speedup_vs_host_route = host_route_ms_scaled / vanhove_accumulate_ms

Usage: batch_vanhove_rate.py [--out PATH] [--parent-lib PATH] [--no-steps] [n:B:origins:nbins[:steps] ...]
Default: 108:4096, 500:1024 and 4000:256, each with 50 and 512 origins and 128 and 1024 bins.  Measurement tool."""
import ctypes as C
import json
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import ljmd_amd  # noqa: E402,F401
from ljmd_amd import BatchEngine, _lib, synthetic  # noqa: E402

REPEATS = 5
SAMPLE = 100
EVERY = 10
SCALED_FROM = 64


def stat(xs, digits=4):
    return round(min(xs), digits), round(max(xs) - min(xs), digits)


def replicas(n, B):
    p, _, _ = synthetic.make_config(n)
    cfg = [synthetic.make_config(n, seed=1000 + b) for b in range(min(B, 64))]
    r = np.stack([cfg[b % len(cfg)][1] for b in range(B)])               # [B, 3, n]
    v = np.stack([cfg[b % len(cfg)][2] for b in range(B)])
    return p, r, v


def timed(call, wait):
    t0 = time.perf_counter()
    call()
    wait()
    return 1e3 * (time.perf_counter() - t0)


def host_route(eng, n, B, max_lag, nbins, rmax, origins):
    """(d): one snapshot against `origins` stored ones, as a user without the feature does it"""
    m = max(1, min(B, SCALED_FROM, 2 ** 25 // (origins * n)))                    # the host's ring stays below 1 GB
    rng = np.random.Generator(np.random.PCG64(3))
    stored = [rng.normal(0.0, 0.05, size=(3, m, n)) for _ in range(origins)]     # the host's own ring
    dr = rmax / nbins
    get_ms, bin_ms = [], []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        ru = np.stack(eng.get_state(("ru",))["ru"])                              # [3, B, n]: every replica comes down
        t1 = time.perf_counter()
        cur = ru[:, :m]
        hist = np.zeros((m, max_lag + 1, nbins + 1), dtype=np.int64)
        s2 = np.zeros((m, max_lag + 1))
        s4 = np.zeros((m, max_lag + 1))
        offs = (np.arange(m) * (nbins + 1))[:, None]
        for e, org in enumerate(stored):
            d = cur - (cur + org)
            r2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
            bins = np.minimum(np.floor(np.sqrt(r2) / dr), nbins).astype(np.int64)
            lag = 1 + e % max_lag
            hist[:, lag] += np.bincount((bins + offs).ravel(), minlength=m * (nbins + 1)).reshape(m, nbins + 1)
            s2[:, lag] += r2.sum(axis=1)
            s4[:, lag] += (r2 * r2).sum(axis=1)
        t2 = time.perf_counter()
        get_ms.append(1e3 * (t1 - t0))
        bin_ms.append(1e3 * (t2 - t1))
    return min(get_ms), min(bin_ms) * B / m, m


def measure(n, B, origins, nbins, steps, off_eng):
    p, r, v = replicas(n, B)
    max_lag = origins if origins < 512 else 511                # 512 ring slots: 511 live origins and the lag-0 entry
    live = min(origins, max_lag)
    rmax = 2.0
    lib = _lib.load()
    out = {"n": n, "replicas": B, "max_lag": max_lag, "origin_stride": 1, "live_origins": live, "nbins": nbins, "rmax": rmax}
    with BatchEngine(p, B) as eng:
        eng.set_state(r[:, 0], r[:, 1], r[:, 2], v[:, 0], v[:, 1], v[:, 2])
        eng.compute_forces()
        wait_vh = lambda: eng._ck(lib.ljmd_batch_vanhove_read(eng._h, None, None, None, None, None))     # noqa: E731
        wait_tcf = lambda: eng._ck(lib.ljmd_batch_tcf_read(eng._h, None, None, None, None))              # noqa: E731
        # (a)
        eng.vanhove_configure(max_lag, 1, nbins, rmax)
        eng.tcf_configure(max_lag, 1)
        for _ in range(max_lag + 1):                           # both rings full
            eng.steps(2, observables=False)
            eng.vanhove_accumulate()
            eng.tcf_accumulate()
        wait_vh()
        wait_tcf()
        vh_ms, tcf_ms = [], []
        for _ in range(REPEATS):
            eng.steps(2, observables=False)
            wait_vh()
            vh_ms.append(timed(eng.vanhove_accumulate, wait_vh))
            tcf_ms.append(timed(eng.tcf_accumulate, wait_tcf))
        counts = np.empty(max_lag + 1, dtype=np.int64)
        r2 = np.empty((B, max_lag + 1))
        eng._ck(lib.ljmd_batch_vanhove_read(eng._h, None, r2.ctypes.data_as(_lib.c_double_p), None,
                                            counts.ctypes.data_as(_lib.c_int64_p), None))
        assert counts[max_lag] > 0 and np.all(np.isfinite(r2)) and r2[:, max_lag].min() > 0.0
        out["vanhove_accumulate_ms"], out["vanhove_accumulate_ms_spread"] = stat(vh_ms)
        out["tcf_accumulate_ms"], out["tcf_accumulate_ms_spread"] = stat(tcf_ms)
        out["ratio_vs_tcf"] = round(min(vh_ms) / min(tcf_ms), 3)
        out["ring_read_GBps"] = round(24.0 * n * B * live / (min(vh_ms) * 1e-3) / 1e9, 1)
        # (d)
        get_ms, bin_ms, m = host_route(eng, n, B, max_lag, nbins, rmax, live)
        out["host_route_ms_scaled"], out["get_state_ms"] = round(get_ms + bin_ms, 1), round(get_ms, 2)
        out["host_route_scaled_from_replicas"] = m
        out["speedup_vs_host_route"] = round((get_ms + bin_ms) / min(vh_ms), 1)
        eng.tcf_configure(0)
        # (b)
        if off_eng is not None:
            eng.vanhove_configure(max_lag, 1, nbins, rmax, every=EVERY)
            for _ in range(-(-(max_lag + 1) * EVERY // steps)):            # the ring full again
                eng.steps(steps, SAMPLE)
            # the feature is switched off by a reconfigure only, which would empty the ring: the off calls run on a second
            # handle of the same size and starting state without the feature, alternating with this one
            on, off, on_prof, off_prof = [], [], None, None
            for _ in range(REPEATS):
                t0 = time.perf_counter()
                eng.steps(steps, SAMPLE)
                on.append(B * steps / (time.perf_counter() - t0))
                if on[-1] == max(on):
                    on_prof = eng.profile_read()
                t0 = time.perf_counter()
                off_eng.steps(steps, SAMPLE)
                off.append(B * steps / (time.perf_counter() - t0))
                if off[-1] == max(off):
                    off_prof = off_eng.profile_read()
            out["steps_per_call"], out["sample_every"], out["vanhove_every"] = steps, SAMPLE, EVERY
            best_on, best_off = max(on), max(off)
            out["vanhove_replica_steps_per_s"], out["vanhove_replica_steps_per_s_spread"] = round(best_on, 1), round(best_on - min(on), 1)
            out["off_replica_steps_per_s"], out["off_replica_steps_per_s_spread"] = round(best_off, 1), round(best_off - min(off), 1)
            out["steps_ratio"] = round(best_on / best_off, 4)
            out["vanhove_kernel_ms"], out["off_kernel_ms"] = round(on_prof["kernel_ms"], 3), round(off_prof["kernel_ms"], 3)
            out["vanhove_launches"], out["off_launches"] = on_prof["launches"], off_prof["launches"]
            out["vanhove_pass_kernel_ms"] = round((on_prof["kernel_ms"] - off_prof["kernel_ms"]) / (steps // EVERY), 4)
    return out



# (c) -- a child process per figure, the C ABI alone, so that the parent commit's library (which lacks the new symbols)
# loads as well
CHILD = r"""
import ctypes as C, sys, time
import numpy as np
lib = C.CDLL(sys.argv[1]); n, B, steps = int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4])
sys.path.insert(0, sys.argv[5])
import ljmd_amd
from ljmd_amd import synthetic
p, _, _ = synthetic.make_config(n)
cfg = [synthetic.make_config(n, seed=1000 + b) for b in range(min(B, 64))]
a = [np.ascontiguousarray(np.stack([cfg[b % len(cfg)][k][ax] for b in range(B)])) for k in (1, 2) for ax in range(3)]
dp = C.POINTER(C.c_double)
lib.ljmd_batch_create.argtypes = [C.POINTER(C.c_void_p), C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_int32, C.c_int32]
lib.ljmd_batch_set_state.argtypes = [C.c_void_p] + [dp] * 6
lib.ljmd_batch_compute_forces.argtypes = [C.c_void_p] + [dp] * 3
lib.ljmd_batch_steps.argtypes = [C.c_void_p, C.c_int32, C.c_int32] + [dp] * 4
lib.ljmd_batch_destroy.argtypes = [C.c_void_p]
h = C.c_void_p()
assert lib.ljmd_batch_create(C.byref(h), B, n, p.box_length, p.dt, p.rc, 0, 0) == 0
assert lib.ljmd_batch_set_state(h, *[x.ctypes.data_as(dp) for x in a]) == 0
assert lib.ljmd_batch_compute_forces(h, None, None, None) == 0
outs = [np.empty((steps // 100, B)) for _ in range(4)]
best = 0.0
for k in range(4):
    t0 = time.perf_counter()
    assert lib.ljmd_batch_steps(h, steps, 100, *[o.ctypes.data_as(dp) for o in outs]) == 0
    if k: best = max(best, B * steps / (time.perf_counter() - t0))
lib.ljmd_batch_destroy(h)
print(best)
"""


def off_rate_against_parent(parent_lib, n, B, steps):
    this_lib = ROOT / "molecular-dynamics-simulation---lennard-jones-monoatomic-fluid_amd" / "libljmd.so"
    series = {"this": [], "parent": [], "parent_again": []}
    for _ in range(REPEATS):
        for name, path in (("this", this_lib), ("parent", parent_lib), ("parent_again", parent_lib)):
            res = subprocess.run([sys.executable, "-c", CHILD, str(path), str(n), str(B), str(steps), str(ROOT)],
                                 check=True, capture_output=True, text=True, timeout=600)
            series[name].append(float(res.stdout.strip().splitlines()[-1]))
    out = {"n": n, "replicas": B, "steps_per_call": steps}
    for name, xs in series.items():
        out[f"off_{name}_steps_per_s"], out[f"off_{name}_steps_per_s_spread"] = round(max(xs), 1), round(max(xs) - min(xs), 1)
    between = abs(out["off_parent_steps_per_s"] - out["off_parent_again_steps_per_s"])
    out["parent_vs_parent"] = round(between, 1)
    out["this_vs_parent"] = round(out["off_this_steps_per_s"] - out["off_parent_steps_per_s"], 1)
    out["agrees_within_parent_spread"] = bool(abs(out["this_vs_parent"]) <= max(between, out["off_parent_steps_per_s_spread"]))
    return out


def main(argv):
    out = ROOT / "profiles" / "batch_vanhove_rate.txt"
    parent_lib, with_steps = None, True
    while argv and argv[0].startswith("--"):
        if argv[0] == "--out":
            out, argv = Path(argv[1]), argv[2:]
        elif argv[0] == "--parent-lib":
            parent_lib, argv = Path(argv[1]), argv[2:]
        elif argv[0] == "--no-steps":
            with_steps, argv = False, argv[1:]
        else:
            raise SystemExit(f"unknown option {argv[0]}")
    default = [(n, B, o, nb) for n, B in ((108, 4096), (500, 1024), (4000, 256)) for o in (50, 512) for nb in (128, 1024)]
    cases = [tuple(map(int, a.split(":"))) for a in argv] or default
    out.parent.mkdir(parents=True, exist_ok=True)
    with open(out, "w") as f:
        def emit(d):
            line = json.dumps(d)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        for case in cases:
            n, B, origins, nbins = case[:4]
            steps = case[4] if len(case) > 4 else (1000 if n < 4000 else 200)
            off_eng = None
            if with_steps:                                     # the handle of the off calls of (b): same state, no feature
                p, r, v = replicas(n, B)
                off_eng = BatchEngine(p, B)
                off_eng.set_state(r[:, 0], r[:, 1], r[:, 2], v[:, 0], v[:, 1], v[:, 2])
                off_eng.compute_forces()
                off_eng.steps(steps, SAMPLE)
            try:
                emit(measure(n, B, origins, nbins, steps, off_eng))
            finally:
                if off_eng is not None:
                    off_eng.close()
        if parent_lib is not None:
            for n, B in sorted({c[:2] for c in cases}):
                emit(off_rate_against_parent(parent_lib, n, B, 1000 if n < 4000 else 200))


if __name__ == "__main__":
    main(sys.argv[1:])
