#!/usr/bin/env python3
"""Cost of the batch engine's on-device density modes (BatchEngine.rhok_*, ljmd_batch_rhok_*), measured in one process on
one card.  One JSON line per case, also written to profiles/batch_rhok_rate.txt (--out PATH for another file).  Every
figure is the MINIMUM of 5 repeats, the repeats of the things compared ALTERNATING, and beside every minimum stands its
spread (max - min of the 5) under the same name with _spread.

  (a) the kernel time of one accumulate -- ljmd_batch_rhok_profile_read, HIP events around the launches of the call --
      for 2, 4 and 8 waves per workgroup (LJMD_BATCH_RHOK_WAVES, read by rhok_configure: the same handle and state are
      reconfigured for every figure, the wave counts taking turns within a repeat)
        accumulate_ms_w2, accumulate_ms_w4, accumulate_ms_w8, best_waves
        terms_per_ns_w*           B n n_modes terms / accumulate_ms
  (b) beside it the kernel time of one step of the same batch, from ljmd_batch_profile_read of steps(STEPS) in the same run
        step_ms, accumulate_over_step_w*
  The last line names the wave counts tried, the one csrc/ljmd_batch_rhok.h keeps (kBatchRhokWaves) and, per case, how far
  the kept one is from the best.

Usage: batch_rhok_rate.py [--out PATH] [n:B:n_modes ...]
Default: 256:1024 with 64, 256 and 1024 modes, and 4096:64 with 256 modes.  Measurement tool."""
import json
import os
import re
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import ljmd_amd  # noqa: E402,F401
from ljmd_amd import BatchEngine, synthetic  # noqa: E402

REPEATS = 5
WAVES = (2, 4, 8)
SNAPSHOTS = 8
STEPS = 20


def stat(xs, digits=5):
    return round(min(xs), digits), round(max(xs) - min(xs), digits)


def replicas(n, B):
    p, _, _ = synthetic.make_config(n)
    cfg = [synthetic.make_config(n, seed=1000 + b) for b in range(min(B, 64))]
    r = np.stack([cfg[b % len(cfg)][1] for b in range(B)])               # [B, 3, n]
    v = np.stack([cfg[b % len(cfg)][2] for b in range(B)])
    return p, r, v


def mode_list(count):
    """the drivers' list grown shell by shell until it holds `count` modes, cut there"""
    from ljmd_amd import Engine
    n2 = 1
    while True:
        modes = Engine.rhok_select_modes(n2, 1 << 20)
        if len(modes) >= count:
            return modes[:count]
        n2 += 1


def accumulate_ms(eng, modes, waves):
    """one accumulate with `waves` waves per workgroup on a freshly configured series -> kernel ms"""
    os.environ["LJMD_BATCH_RHOK_WAVES"] = str(waves)
    try:
        eng.rhok_configure(modes, SNAPSHOTS)
    finally:
        del os.environ["LJMD_BATCH_RHOK_WAVES"]
    eng.rhok_accumulate()                                      # the first launch of a configuration is not timed
    eng.rhok_accumulate()
    return eng.rhok_profile()["kernel_ms"]


def measure(n, B, n_modes):
    p, r, v = replicas(n, B)
    modes = mode_list(n_modes)
    out = {"n": n, "replicas": B, "n_modes": n_modes, "snapshots_room": SNAPSHOTS}
    with BatchEngine(p, B) as eng:
        eng.set_state(r[:, 0], r[:, 1], r[:, 2], v[:, 0], v[:, 1], v[:, 2])
        eng.compute_forces()
        eng.steps(STEPS, observables=False)
        ms = {w: [] for w in WAVES}
        step_ms = []
        for _ in range(REPEATS):
            for w in WAVES:
                ms[w].append(accumulate_ms(eng, modes, w))
            eng.rhok_configure(modes, 0)
            eng.steps(STEPS, observables=False)
            step_ms.append(eng.profile_read()["kernel_ms"] / STEPS)
        # the words do not depend on the wave count
        words = {}
        for w in WAVES:
            accumulate_ms(eng, modes, w)
            words[w] = eng.rhok_read_exact(raw=True)[0]
        assert all(np.array_equal(words[w], words[WAVES[0]]) for w in WAVES)
        assert words[WAVES[0]].any()
    out["step_ms"], out["step_ms_spread"] = stat(step_ms)
    for w in WAVES:
        out[f"accumulate_ms_w{w}"], out[f"accumulate_ms_w{w}_spread"] = stat(ms[w])
        out[f"terms_per_ns_w{w}"] = round(1e-6 * B * n * n_modes / min(ms[w]), 2)
        out[f"accumulate_over_step_w{w}"] = round(min(ms[w]) / min(step_ms), 3)
    out["best_waves"] = min(WAVES, key=lambda w: min(ms[w]))
    return out


def kept_waves():
    text = (ROOT / "molecular-dynamics-simulation---lennard-jones-monoatomic-fluid_amd" / "csrc" / "ljmd_batch_rhok.h").read_text()
    return int(re.search(r"kBatchRhokWaves = (\d+);", text).group(1))


def main(argv):
    out = ROOT / "profiles" / "batch_rhok_rate.txt"
    while argv and argv[0].startswith("--"):
        if argv[0] == "--out":
            out, argv = Path(argv[1]), argv[2:]
        else:
            raise SystemExit(f"unknown option {argv[0]}")
    default = [(256, 1024, 64), (256, 1024, 256), (256, 1024, 1024), (4096, 64, 256)]
    cases = [tuple(map(int, a.split(":"))) for a in argv] or default
    out.parent.mkdir(parents=True, exist_ok=True)
    kept = kept_waves()
    with open(out, "w") as f:
        def emit(d):
            line = json.dumps(d)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        results = []
        for case in cases:
            results.append(measure(*case))
            emit(results[-1])
        emit({"waves_tried": list(WAVES), "waves_kept": kept,
              "kept_over_best": {f"{r['n']}:{r['replicas']}:{r['n_modes']}":
                                 round(r[f"accumulate_ms_w{kept}"] / r[f"accumulate_ms_w{r['best_waves']}"], 3) for r in results}})


if __name__ == "__main__":
    main(sys.argv[1:])
