"""CPU-only: which k-d levels of a re-sort the finishing kernel takes (LaunchPlan::kd_finish_from), and
why its order is the library sort's.

tests/kd_plan_host prints the level tables plan_engine builds (host code under ASan and UBSan).  They are held against a
restatement in numpy of the halving, the cap decision is pinned for the shapes the GPU tests run (n = 33000 is there
because its 65-tile segments, 4160 slots, sit just above the cap at level 3 while level 4 fits), and a numpy model of the
level loop -- a stable argsort per level on the integer keys (segment << 24) | coordinate -- is held against a model of the
kernel: the levels above by that argsort, then every segment of the first level inside the cap on its own, ordering the
64-bit words (sub-segment, coordinate, current position, position at the start) by plain value."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

HERE = ROOT / "tests" / "kd_plan_host"
TILE, CAP, MAX_LEVELS = 64, 4096, 6
SHAPES = {24576: 3, 32768: 3, 33000: 4, 262144: 6, 1000: 0, 4096: 0, 4160: 1}      # n -> first level inside the kernel


def plans(extra_env=None):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc absent: the program cannot be built")
    subprocess.run(["make", "-C", str(HERE)], check=True, capture_output=True, timeout=600)
    env = {k: v for k, v in os.environ.items() if not k.startswith("LJMD_")}
    env.update(FAKEHIP_DEVICES="1", ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:exitcode=23",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1:exitcode=24")
    env.update(extra_env or {})
    out = subprocess.run([str(HERE / "kd_plan_host")] + [str(n) for n in SHAPES], env=env, capture_output=True, timeout=120)
    stderr = out.stderr.decode(errors="replace")
    assert out.returncode == 0, stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in stderr and "runtime error:" not in stderr, stderr[-4000:]
    return {p["n"]: p for p in map(json.loads, out.stdout.decode().splitlines())}


@pytest.fixture(scope="module")
def default_plans():
    return plans()


def level_tables(S):
    """segments = runs of whole tiles, halved (lower half rounded up) until every segment is one tile"""
    tiles = -(-S // TILE)
    bounds, out = [0, tiles], []
    while any(b - a > 1 for a, b in zip(bounds, bounds[1:])):
        out.append([min(b * TILE, S) for b in bounds])
        nxt = []
        for a, b in zip(bounds, bounds[1:]):
            nxt.append(a)
            if b - a > 1:
                nxt.append(a + (b - a + 1) // 2)
        bounds = nxt + [tiles]
    return out


def test_level_tables_and_cap_decision(default_plans):
    for n, want_from in SHAPES.items():
        p = default_plans[n]
        assert (p["cap"], p["max_levels"]) == (CAP, MAX_LEVELS)
        levels = level_tables(p["S"])
        assert p["levels"] == levels, n
        largest = [max(np.diff(b)) for b in levels]
        fits = [l for l, m in enumerate(largest) if m <= CAP]
        assert p["kd_finish_from"] == (fits[0] if fits else len(levels)) == want_from, (n, largest)
        assert all(m <= CAP for m in largest[want_from:]) and all(m > CAP for m in largest[:want_from]), n
        assert len(levels) - want_from <= MAX_LEVELS, n                   # one launch finishes the re-sort
    largest = [max(np.diff(b)) for b in default_plans[33000]["levels"]]
    assert largest[3] == 65 * TILE and largest[4] == 33 * TILE           # just above the cap, then below it
    assert max(np.diff(default_plans[32768]["levels"][3])) == CAP        # exactly the cap


def test_knob_keeps_every_level_on_the_library_path():
    for n, p in plans({"LJMD_KD_SORT": "cub"}).items():
        assert p["kd_finish_from"] == len(p["levels"]), n


def library_levels(q, levels, axes, idx, upto):
    for l in range(upto):
        seg = np.searchsorted(levels[l], np.arange(len(idx)), side="right") - 1
        key = (seg.astype(np.uint64) << np.uint64(24)) | q[axes[l]][idx]
        idx = idx[np.argsort(key, kind="stable")]
    return idx


def finishing_kernel(q, levels, axes, idx, first):
    idx = idx.copy()
    for lo, hi in zip(levels[first], levels[first][1:]):                 # one workgroup each
        home_idx = idx[lo:hi].copy()                                     # the slice as loaded; it stays in place
        home = np.arange(hi - lo, dtype=np.uint64)
        pos = np.arange(hi - lo, dtype=np.uint64)
        for l in range(first, len(levels)):
            bounds = [b - lo for b in levels[l] if lo <= b <= hi]
            assert bounds[0] == 0 and bounds[-1] == hi - lo and len(bounds) - 1 <= CAP // TILE
            sub = (np.searchsorted(bounds[:-1], pos, side="right") - 1).astype(np.uint64)
            word = (sub << np.uint64(56)) | (q[axes[l]][home_idx[home.astype(np.int64)]] << np.uint64(32)) | (pos << np.uint64(16)) | home
            assert len(np.unique(word)) == len(word)                     # distinct: any sorting network leaves one order
            home = np.sort(word) & np.uint64(0xffff)
        idx[lo:hi] = home_idx[home.astype(np.int64)]
    return idx


@pytest.mark.parametrize("n", [24576, 32768, 33000, 4160])
@pytest.mark.parametrize("spread", [37, 1 << 24])
def test_finishing_kernel_model_equals_the_level_loop(default_plans, n, spread):
    """spread = 37: a few dozen distinct coordinates, so nearly every comparison is a tie the stable order decides"""
    p = default_plans[n]
    levels, S = p["levels"], p["S"]
    rng = np.random.default_rng(n + spread)
    q = rng.integers(0, spread, size=(3, S)).astype(np.uint64)
    axes = [l % 3 for l in range(len(levels))]
    want = library_levels(q, levels, axes, np.arange(S), len(levels))
    upper = library_levels(q, levels, axes, np.arange(S), p["kd_finish_from"])
    got = finishing_kernel(q, levels, axes, upper, p["kd_finish_from"])
    assert np.array_equal(got, want)
