"""GPU tests of the two-launch pair kernel with the two-phase slab reduction (LJMD_REDUCE_SPLIT).

The path is on by default only for large one-rank fp64 systems; LJMD_REDUCE_SPLIT=k forces it at the sizes used here
(k of the pair kernel's S slices go to the second launch).  n = 32768 is the smallest size with 4-tile row groups and
many slices (S = 130, two slices per offset); n = 33000 adds padding slots and a partially filled last tile.  What
must hold: the pair kernel's work items do not depend on the launch that runs them, so the three potential-energy
scalars of a force call are BITWISE those of the unsplit path; the accelerations are a re-associated sum of the same
terms and stay within the bound the parity tests use against the oracle."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from ljmd_amd import Engine, synthetic
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

N = 32768
S_SLICES = 130                      # slices of the pair kernel at n = 32768 (ljmd_plan.cpp)
REL_ACCEL = 1e-12                   # tests/test_gpu_parity.py, single force call
SPLITS = (1, S_SLICES // 2, S_SLICES - 1)


def force_call(p, r, v, split, monkeypatch):
    monkeypatch.setenv("LJMD_REDUCE_SPLIT", str(split))
    with Engine(p) as eng:
        eng.set_state(r[0], r[1], r[2], v[0], v[1], v[2])
        assert eng.pair_kernel_name() == "pair_n3_kernel"
        sc = eng.compute_forces()
        a = np.stack(eng.get_state(("a",))["a"])
    return sc, a


@pytest.fixture(scope="module")
def oracle_n32768(oracle):
    p, r, v = synthetic.make_config(N, seed=77)
    po = oracle.derive_params(N, p.box_length, p.dt, p.rc)
    e, d, dd, ax, ay, az = oracle.compute_forces(po, r[0].copy(), r[1].copy(), r[2].copy())
    a = np.stack([ax, ay, az])
    a.setflags(write=False)
    return p, r, v, (e, d, dd), a


def test_force_call_split_vs_unsplit_and_oracle_n32768(oracle_n32768, monkeypatch):
    p, r, v, sc_o, a_o = oracle_n32768
    sc0, a0 = force_call(p, r, v, 0, monkeypatch)
    amax = np.abs(a_o).max()
    print("split 0: max|a - a_oracle| / max|a| = %.3e" % (np.abs(a0 - a_o).max() / amax))
    assert np.abs(a0 - a_o).max() <= REL_ACCEL * amax
    for k in SPLITS:
        sc, a = force_call(p, r, v, k, monkeypatch)
        print("split %d: max|a - a_oracle| / max|a| = %.3e, against split 0 %.3e"
              % (k, np.abs(a - a_o).max() / amax, np.abs(a - a0).max() / amax))
        assert sc == sc0, (k, sc, sc0)                              # epot, d_epot, dd_epot: bit for bit
        assert np.abs(a - a_o).max() <= REL_ACCEL * amax, k
        assert np.abs(a - a0).max() <= REL_ACCEL * amax, k
    for x, y in zip(sc0, sc_o):
        assert abs(x - y) <= 1e-12 * abs(y)


def test_ragged_size_vs_oracle_n33000(oracle, monkeypatch):
    n = 33000
    p, r, v = synthetic.make_config(n, seed=3)
    po = oracle.derive_params(n, p.box_length, p.dt, p.rc)
    e_o, d_o, dd_o, ax, ay, az = oracle.compute_forces(po, r[0].copy(), r[1].copy(), r[2].copy())
    a_o = np.stack([ax, ay, az])
    sc0, a0 = force_call(p, r, v, 0, monkeypatch)
    for k in (1, 40):
        sc, a = force_call(p, r, v, k, monkeypatch)
        print("n = 33000, split %d: max|a - a_oracle| / max|a| = %.3e" % (k, np.abs(a - a_o).max() / np.abs(a_o).max()))
        assert sc == sc0
        assert np.abs(a - a_o).max() <= REL_ACCEL * np.abs(a_o).max()
        for x, y in zip(sc, (e_o, d_o, dd_o)):
            assert abs(x - y) <= 1e-12 * abs(y)


def trajectory(p, r, v, steps, sampled=False):
    with Engine(p) as eng:
        eng.set_state(r[0], r[1], r[2], v[0], v[1], v[2])
        eng.compute_forces()
        if sampled:
            eng.enqueue_steps(steps, sampled=True)
            sc = np.stack(eng.collect_steps(steps))
        else:
            sc = np.stack(eng.verlet_steps(steps))                   # rows epot, ekin, d_epot, dd_epot
        st = {k: np.stack(x) for k, x in eng.get_state().items()}
    return sc, st


def test_steps_with_a_resort_are_deterministic_and_keep_etot(monkeypatch):
    """25 steps with re-sorts every 10: two runs with the split on are bitwise equal in r, ru, v, a and the four series,
    and Etot stays within 1e-10 of the unsplit run (the trajectory band of tests/test_gpu_parity.py)."""
    p, r, v = synthetic.make_config(N, seed=11)
    monkeypatch.setenv("LJMD_RESORT_EVERY", "10")
    monkeypatch.setenv("LJMD_REDUCE_SPLIT", "0")
    sc_off, _ = trajectory(p, r, v, 25)
    monkeypatch.setenv("LJMD_REDUCE_SPLIT", str(S_SLICES // 8))
    sc_a, st_a = trajectory(p, r, v, 25)
    sc_b, st_b = trajectory(p, r, v, 25)
    assert np.array_equal(sc_a, sc_b)
    for key in ("r", "ru", "v", "a"):
        assert np.array_equal(st_a[key], st_b[key]), key
    etot_on, etot_off = sc_a[0] + sc_a[1], sc_off[0] + sc_off[1]
    print("max rel Etot difference, split on vs off, 25 steps: %.3e" % np.max(np.abs(etot_on - etot_off) / np.abs(etot_off)))
    assert np.max(np.abs(etot_on - etot_off) / np.abs(etot_off)) <= 1e-10


def test_sampled_segment_equals_every_step_path(monkeypatch):
    """ljmd_enqueue_steps_sampled with the split on: r, ru, v, a, ekin and the sampled step's scalars bitwise those of
    the every-step path with the split on; NaN on the unsampled steps."""
    p, r, v = synthetic.make_config(N, seed=11)
    monkeypatch.setenv("LJMD_REDUCE_SPLIT", str(S_SLICES // 8))
    want, st = trajectory(p, r, v, 8)
    got, fin = trajectory(p, r, v, 8, sampled=True)
    assert np.array_equal(got[1], want[1])                           # ekin, every step
    assert np.array_equal(got[:, -1], want[:, -1])                   # the sampled step, all four
    assert np.all(np.isnan(got[[0, 2, 3], :-1]))
    for key in ("r", "ru", "v", "a"):
        assert np.array_equal(fin[key], st[key]), key


@pytest.mark.parametrize("case,env,extra", [("fp64_split_0", {"LJMD_REDUCE_SPLIT": "0"}, []),
                                            ("mixed_split_asked", {"LJMD_REDUCE_SPLIT": "16"}, ["--mode", "mixed"])])
def test_path_off_reproduces_the_recorded_outputs(case, env, extra, tmp_path):
    """With the path off -- LJMD_REDUCE_SPLIT=0, or the mixed mode whatever the knob says -- a short bench run at n = 32768
    writes, file for file, what the commit before this path wrote (SHA-256 of every file of --dump-outputs, recorded with
    that commit's library on an MI355X: tests/golden/reduce_split_off_n32768.json)."""
    want = json.loads((GOLDEN / "reduce_split_off_n32768.json").read_text())[case]
    e = {k: v for k, v in os.environ.items() if not k.startswith("LJMD_")}
    e.update(env)
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "1", "--particles", str(N),
           "--dump-outputs", str(tmp_path)] + extra
    subprocess.run(cmd, check=True, env=e, capture_output=True, timeout=300, cwd=str(ROOT))
    got = {f.name: hashlib.sha256(f.read_bytes()).hexdigest() for f in sorted(tmp_path.iterdir())}
    assert got == want
