#!/usr/bin/env python3
"""Cost of preparing a batch's initial configurations on the device (BatchEngine.prepare, ljmd_batch_prepare) against
the route through the host at the same commit.  One JSON line per (n, B), also written to
profiles/batch_prepare_rate.txt (--out PATH for another file).  n must be 4 k^3.

  (a) on the device: prepare(seeds 1 .. B, target -4.6 n, warmup_steps=0) on one handle
        prepare_ms               wall time of the call: lattice, velocities, centre of mass, one force call, one kinetic
                                 energy call, the scaling
        forces_kinetic_ms        wall time of compute_forces() + kinetic_energy() on the prepared state: the part of
                                 prepare_ms that any route pays
        init_and_scale_ms        prepare_ms - forces_kinetic_ms: what the two new kernels and their copies cost
  (b) through the host: per replica one process of bin/md_init_replay rv -- the product's host arithmetic of the
      initial-configuration program (lattice, generator, centre of mass, scaling) given the lattice energy, no GPU
      involved -- timed on the first 64 replicas and SCALED by B / 64 (host_init_ms_scaled); then the files read back,
      set_state of all B replicas, compute_forces and kinetic_energy (host_upload_forces_ms, timed in full).
      md_init_replay has the reference's seed hard-wired, as md_initial_config_gpu has, so every host replica is the
      same system; md_initial_config_gpu itself also creates an engine and calls the GPU twice per process, so the
      host route measured here is a lower bound of the route a user has today.
        host_route_ms_scaled     host_init_ms_scaled + host_upload_forces_ms
        speedup_vs_host_route    host_route_ms_scaled / prepare_ms

Usage: batch_prepare_rate.py [--out PATH] [--timeout SECONDS] [n:B ...]   Default: 108:4096 500:1024 4000:256.
Every case runs in a child process of its own under its own time limit (default 300 s); after a case that fails or
runs out of time no further case is started.  Each device figure is the time per call over the best of three windows
of at least 0.25 s of back-to-back calls, after a warm-up call.
Measurement tool."""
import json
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
PKG = ROOT / "molecular-dynamics-simulation---lennard-jones-monoatomic-fluid_amd"
sys.path.insert(0, str(ROOT))

SCALED_FROM = 64
WINDOW_S = 0.25
TARGET_PER_PARTICLE = -4.6


def best_ms(call, repeats=3):
    """milliseconds per call: the best of `repeats` windows of at least WINDOW_S seconds of back-to-back calls (every
    call timed here ends in a device synchronise)"""
    t0 = time.perf_counter()
    call()
    inner = max(1, min(5000, int(WINDOW_S / max(time.perf_counter() - t0, 1e-6)) + 1))
    best = float("inf")
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(inner):
            call()
        best = min(best, 1e3 * (time.perf_counter() - t0) / inner)
    return best


def measure(n, B):
    import ljmd_amd  # noqa: F401
    from ljmd_amd import BatchEngine, io_formats, md_types, synthetic

    k = round((n / 4.0) ** (1.0 / 3.0))
    assert 4 * k ** 3 == n, f"n = {n} is not 4 k^3"
    L = synthetic.box_length(n)
    p = md_types.init_params(n, L, 0.005, 0.49 * L)
    target = TARGET_PER_PARTICLE * n
    seeds = np.arange(1, B + 1)
    replay = PKG / "bin" / "md_init_replay"
    assert replay.exists(), "build the Fortran tools first"
    with BatchEngine(p, B) as eng, tempfile.TemporaryDirectory() as tmp:
        epot0, ekin0 = eng.prepare(seeds, target)                          # warm-up call
        assert np.all(target - epot0 > 0) and np.all(ekin0 > 0)
        prepare_ms = best_ms(lambda: eng.prepare(seeds, target))
        forces_ms = best_ms(lambda: (eng.compute_forces(), eng.kinetic_energy()))
        v = eng.get_state(("v",))["v"]
        assert np.all(np.isfinite(v[0])) and (B == 1 or not np.array_equal(v[0][0], v[0][B - 1]))

        # (b) the host route
        tmp = Path(tmp)
        (tmp / "inputs").mkdir()
        (tmp / "inputs" / "input_simulation_parameters.txt").write_text(
            f"k   total_steps   output_interval   warmup_steps\n{k}   10   1   0\n\n"
            f"dt        L     rc_over_L\n0.005   {L!r}   0.49\n\ntarget_total_energy\n{target!r}\n")
        np.array([epot0[0]]).tofile(tmp / "epot.bin")
        m = min(B, SCALED_FROM)
        t0 = time.perf_counter()
        for b in range(m):
            subprocess.run([str(replay), "rv", "epot.bin", f"rv_{b}.dat"], cwd=tmp, check=True, timeout=60)
        host_init_ms = 1e3 * (time.perf_counter() - t0)

        def upload():
            rv = [io_formats.read_rv_init(tmp / f"rv_{b}.dat", n) for b in range(m)]
            r = np.stack([rv[b % m][0] for b in range(B)])                  # [B, 3, n]
            vv = np.stack([rv[b % m][1] for b in range(B)])
            eng.set_state(r[:, 0], r[:, 1], r[:, 2], vv[:, 0], vv[:, 1], vv[:, 2])
            eng.compute_forces()
            eng.kinetic_energy()
        upload_ms = best_ms(upload)
    host_scaled = host_init_ms * B / m
    return {"n": n, "replicas": B, "warmup_steps": 0,
            "prepare_ms": round(prepare_ms, 3), "forces_kinetic_ms": round(forces_ms, 3),
            "init_and_scale_ms": round(prepare_ms - forces_ms, 3),
            "prepared_replicas_per_s": round(B / (prepare_ms * 1e-3), 1),
            "host_init_per_replica_ms": round(host_init_ms / m, 3), "host_init_scaled_from_replicas": m,
            "host_init_ms_scaled": round(host_scaled, 1), "host_upload_forces_ms": round(upload_ms, 3),
            "host_route_ms_scaled": round(host_scaled + upload_ms, 1),
            "speedup_vs_host_route": round((host_scaled + upload_ms) / prepare_ms, 1)}


def main(argv):
    if argv[:1] == ["--case"]:                                              # the child: one case, one JSON line
        n, B = map(int, argv[1].split(":"))
        print(json.dumps(measure(n, B)), flush=True)
        return 0
    out, limit = ROOT / "profiles" / "batch_prepare_rate.txt", 300
    while argv[:1] in (["--out"], ["--timeout"]):
        if argv[0] == "--out":
            out = Path(argv[1])
        else:
            limit = int(argv[1])
        argv = argv[2:]
    cases = argv or ["108:4096", "500:1024", "4000:256"]
    out.parent.mkdir(parents=True, exist_ok=True)
    with open(out, "w") as f:
        for case in cases:
            try:
                child = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--case", case],
                                       capture_output=True, text=True, timeout=limit)
            except subprocess.TimeoutExpired:
                print(f"case {case}: no result within {limit} s; stopping", file=sys.stderr)
                return 124
            if child.returncode != 0:
                print(f"case {case}: exit status {child.returncode}; stopping\n{child.stderr[-4000:]}", file=sys.stderr)
                return child.returncode if child.returncode > 0 else 1
            line = child.stdout.strip().splitlines()[-1]
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
