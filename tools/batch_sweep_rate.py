#!/usr/bin/env python3
"""Aggregate step rate of a sweep over state points in ONE batch handle whose replicas each have their own
(n, L, dt, rc) (BatchEngine.per_replica, ljmd_batch_create_per_replica) against one homogeneous handle per state point
stepped one after another (BatchEngine, ljmd_batch_create), measured in the same process on the same card, best of 3.
One JSON line per measurement:

  (a) density sweep: n = 500, 16 densities rho = 0.50 .. 0.95, rc = 0.49 L, 16 runs each (B = 256), 1000 steps,
      sample_every = 100
  (b) size sweep: k = 3 .. 10 (n = 108 .. 4000), 32 runs each (B = 256), 100 steps, sample_every = 100; the one handle
      with its kernel-class groups on streams of their own (the default) and one after another
      (LJMD_BATCH_GROUP_STREAMS=0), beside the kernel time of every per-size handle
  (c) regression: the three B > 1 lines of tools/batch_rate.py, re-run here

replica_steps_per_s = replicas x steps / wall time of the ljmd_batch_steps call(s); kernel_ms = HIP-event time of the
call(s) (ljmd_batch_profile_read).  Usage: batch_sweep_rate.py [a] [b] [c] (default all).  Measurement tool."""
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))
import ljmd_amd  # noqa: E402,F401
from ljmd_amd import BatchEngine, synthetic  # noqa: E402

SAMPLE = 100


def _configs(points, runs):
    """points: [(n, rho)] -> per state point `runs` distinct configurations (rc = 0.49 L, dt = 0.005)"""
    return [[synthetic.make_config(n, seed=1000 + 97 * j + i, rho=rho) for i in range(runs)]
            for j, (n, rho) in enumerate(points)]


def _time_steps(engines, steps):
    """best of 3 of stepping every engine once, one after another -> (wall s, [kernel ms per engine], launches)"""
    for eng in engines:
        eng.steps(SAMPLE, SAMPLE)                                     # warm-up
    best = None
    for _ in range(3):
        t0 = time.perf_counter()
        for eng in engines:
            e, k, _, _ = eng.steps(steps, SAMPLE)
        wall = time.perf_counter() - t0
        if best is None or wall < best[0]:
            prof = [eng.profile_read() for eng in engines]
            best = (wall, [q["kernel_ms"] for q in prof], sum(q["launches"] for q in prof))
        assert np.all(np.isfinite(e)) and np.all(np.isfinite(k))
    return best


def _one_handle(groups, steps):
    flat = [c for g in groups for c in g]
    eng = BatchEngine.per_replica([c[0] for c in flat])
    eng.set_state(*[[c[1][ax] for c in flat] for ax in range(3)], *[[c[2][ax] for c in flat] for ax in range(3)])
    eng.compute_forces()
    wall, ms, launches = _time_steps([eng], steps)
    eng.close()
    return len(flat) * steps / wall, ms[0], launches


def _per_point_handles(groups, steps):
    engines = []
    for g in groups:
        eng = BatchEngine(g[0][0], len(g))
        r = np.stack([c[1] for c in g])
        v = np.stack([c[2] for c in g])
        eng.set_state(r[:, 0], r[:, 1], r[:, 2], v[:, 0], v[:, 1], v[:, 2])
        eng.compute_forces()
        engines.append(eng)
    wall, ms, launches = _time_steps(engines, steps)
    for eng in engines:
        eng.close()
    return sum(len(g) for g in groups) * steps / wall, ms, launches


def _emit(**kw):
    print(json.dumps(kw), flush=True)


def density_sweep():
    rhos = [round(0.50 + 0.03 * j, 2) for j in range(16)]
    groups = _configs([(500, rho) for rho in rhos], 16)
    one, one_ms, one_l = _one_handle(groups, 1000)
    many, many_ms, many_l = _per_point_handles(groups, 1000)
    _emit(case="a_density_sweep", n=500, rho=[rhos[0], rhos[-1]], state_points=16, runs_each=16, steps=1000,
          sample_every=SAMPLE, one_handle_replica_steps_per_s=round(one, 1), one_handle_kernel_ms=round(one_ms, 3),
          one_handle_launches=one_l, per_point_replica_steps_per_s=round(many, 1),
          per_point_kernel_ms_sum=round(sum(many_ms), 3), per_point_launches=many_l, speedup=round(one / many, 2))


def size_sweep():
    ks = list(range(3, 11))
    groups = _configs([(4 * k ** 3, 0.8) for k in ks], 32)
    os.environ["LJMD_BATCH_GROUP_STREAMS"] = "0"
    serial, serial_ms, serial_l = _one_handle(groups, 100)
    del os.environ["LJMD_BATCH_GROUP_STREAMS"]
    one, one_ms, one_l = _one_handle(groups, 100)
    many, many_ms, many_l = _per_point_handles(groups, 100)
    _emit(case="b_size_sweep", k=[ks[0], ks[-1]], runs_each=32, steps=100, sample_every=SAMPLE,
          one_handle_replica_steps_per_s=round(one, 1), one_handle_kernel_ms=round(one_ms, 3),
          one_handle_launches=one_l, one_handle_serial_groups_replica_steps_per_s=round(serial, 1),
          one_handle_serial_groups_kernel_ms=round(serial_ms, 3),
          per_size_replica_steps_per_s=round(many, 1), per_size_kernel_ms_sum=round(sum(many_ms), 3),
          per_size_kernel_ms={str(4 * k ** 3): round(m, 3) for k, m in zip(ks, many_ms)}, per_size_launches=many_l,
          speedup=round(one / many, 2), speedup_serial_groups=round(serial / many, 2))


def regression():
    import batch_rate
    committed = {}
    path = Path(__file__).resolve().parent.parent / "profiles" / "batch_replicas_rate.txt"
    for line in path.read_text().splitlines():
        if line.startswith("{"):
            d = json.loads(line)
            committed[(d["n"], d["replicas"])] = d["batch_replica_steps_per_s"]
    for n, B, steps in ((108, 4096, 1000), (500, 1024, 1000), (4000, 256, 100)):
        rate, prof = batch_rate.batch_rate(n, B, steps)
        ref = committed.get((n, B))
        _emit(case="c_regression", n=n, replicas=B, steps_per_call=steps, sample_every=SAMPLE,
              batch_replica_steps_per_s=round(rate, 1), launches_per_call=prof["launches"],
              kernel_ms_per_call=round(prof["kernel_ms"], 3), committed_replica_steps_per_s=ref,
              vs_committed_pct=round(100.0 * (rate / ref - 1.0), 2) if ref else None)


def main(argv):
    which = argv or ["a", "b", "c"]
    for w in which:
        {"a": density_sweep, "b": size_sweep, "c": regression}[w]()


if __name__ == "__main__":
    main(sys.argv[1:])
