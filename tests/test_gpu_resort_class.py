"""GPU tests of the re-sort with its lower k-d levels in one launch (kd_finish_kernel) and one gather.

The permutation a re-sort leaves must be the library sort's for every input, so every output bit stays what it was.  All
runs re-sort every 2 steps (LJMD_RESORT_EVERY=2): three re-sorts fall inside six steps, besides the one at set_state.
Shapes: n = 24576 (2-tile row groups; the level with 48-tile segments is the first inside the kernel), n = 32768 (4-tile
row groups; 64-tile segments, exactly the 4096 slots one workgroup sorts), n = 33000 (ragged last tile, uneven segments:
65 tiles = 4160 slots at level 3 stay with the library, 33 tiles at level 4 go to the kernel)."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from ljmd_amd import Engine, synthetic
from ljmd_amd import _lib as _abi
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

CASES = {
    "n24576_fp64": (24576, {}, "fp64"),
    "n32768_fp64": (32768, {}, "fp64"),
    "n32768_mixed": (32768, {}, "mixed"),
    "n33000_fp64": (33000, {}, "fp64"),
    "n33000_fp64_split40": (33000, {"LJMD_REDUCE_SPLIT": "40"}, "fp64"),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_outputs_reproduce_the_parent_record(case, tmp_path):
    """A six-step bench run writes, file for file, what the commit before this kernel wrote (SHA-256 of every file of
    --dump-outputs, recorded with that commit's library on an MI355X: tests/golden/resort_class_parent.json)."""
    n, env, mode = CASES[case]
    want = json.loads((GOLDEN / "resort_class_parent.json").read_text())[case]
    e = {k: v for k, v in os.environ.items() if not k.startswith("LJMD_")}
    e["LJMD_RESORT_EVERY"] = "2"
    e.update(env)
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "2", "--particles", str(n),
           "--dump-outputs", str(tmp_path)] + (["--mode", "mixed"] if mode == "mixed" else [])
    subprocess.run(cmd, check=True, env=e, capture_output=True, timeout=300, cwd=str(ROOT))
    got = {f.name: hashlib.sha256(f.read_bytes()).hexdigest() for f in sorted(tmp_path.iterdir())}
    assert got == want


def six_steps(n, mode):
    p, r, v = synthetic.make_config(n, seed=5)
    kw = {"precision_mode": _abi.PRECISION_FP32_FORCE} if mode == "mixed" else {}
    with Engine(p, **kw) as eng:
        eng.set_state(r[0], r[1], r[2], v[0], v[1], v[2])
        eng.compute_forces()
        sc = np.stack(eng.verlet_steps(6))
        st = {k: np.stack(x) for k, x in eng.get_state().items()}
    return sc, st


@pytest.mark.parametrize("case", sorted(CASES))
def test_library_sort_and_finishing_kernel_agree(case, monkeypatch):
    """LJMD_KD_SORT=cub (every level a library sort) against the default: the four per-step series and r, ru, v, a, which
    reach the caller through the slot -> particle permutation, are equal bit for bit."""
    n, env, mode = CASES[case]
    monkeypatch.setenv("LJMD_RESORT_EVERY", "2")
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    monkeypatch.setenv("LJMD_KD_SORT", "cub")
    sc_cub, st_cub = six_steps(n, mode)
    monkeypatch.delenv("LJMD_KD_SORT")
    sc, st = six_steps(n, mode)
    assert np.array_equal(sc, sc_cub)
    for key in ("r", "ru", "v", "a"):
        assert np.array_equal(st[key], st_cub[key]), key
