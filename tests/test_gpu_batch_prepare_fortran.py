"""-m gpu: bin/md_simulation_many_gpu with LJMD_SEED_BASE -- every run prepared on the device (ljmd_batch_prepare) instead
of read from an rv_init.dat.  The golden input of the reference's initial-configuration program (k = 3, target -500,
10 steps, every step written) with LJMD_RUNS=3 LJMD_SEED_BASE=12345: run 1 has the reference's seed, so its
rv_init_gpu.dat is compared with the reference's rv_init.dat; the runs differ; and each run is byte-identical to a
single run with its seed."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from ljmd_amd import BatchEngine, io_formats, md_types
from test_batch_prepare_host import GOLDEN_INPUTS

pytestmark = pytest.mark.gpu

PKG = ROOT / "molecular-dynamics-simulation---lennard-jones-monoatomic-fluid_amd"
NAME = "init_k3_warm0"
SEED_BASE = 12345


def _run(workdir, runs, seed_base):
    """-> {run number: {file name: bytes}}; no rv_init.dat exists anywhere under workdir"""
    exe = PKG / "bin" / "md_simulation_many_gpu"
    assert exe.exists(), "run __graft_entry__.build() first"
    (workdir / "inputs").mkdir(parents=True)
    shutil.copy(GOLDEN / NAME / "input_simulation_parameters.txt", workdir / "inputs")
    (workdir / "outputs").mkdir()
    env = {k: v for k, v in os.environ.items() if not k.startswith("LJMD_") or k in ("LJMD_DEVICE", "LJMD_LIBRARY")}
    out = subprocess.run([str(exe)], cwd=workdir, check=True, capture_output=True, text=True, timeout=300,
                         env=dict(env, LJMD_RUNS=str(runs), LJMD_SEED_BASE=str(seed_base)))
    assert "rv_init.dat" not in out.stdout
    return {i: {f.name: f.read_bytes() for f in (workdir / "outputs" / f"run_{i:04d}").iterdir()}
            for i in range(1, runs + 1)}


def test_seed_base_prepares_independent_runs(tmp_path):
    n, L, rc, target = GOLDEN_INPUTS[NAME]
    many = _run(tmp_path / "many", 3, SEED_BASE)
    for files in many.values():
        assert {"rv_init_gpu.dat", "rva.dat", "instantaneous_energies.dat", "md_final_results.txt"} <= set(files)
        assert "rv_init.dat" not in files
    # run 1 has the reference's seed: the bounds of the library test against the reference's rv_init.dat.  The driver
    # does not print epot0; a replica's result depends on nothing but its own parameters, so a handle of the same
    # system returns the same epot0
    r, v = io_formats.read_rv_init(tmp_path / "many" / "outputs" / "run_0001" / "rv_init_gpu.dat", n)
    r_ref, v_ref = io_formats.read_rv_init(GOLDEN / NAME / "rv_init.dat", n)
    epot_ref = float(np.fromfile(GOLDEN / NAME / "epot.bin", dtype=np.float64)[0])
    assert r.tobytes() == r_ref.tobytes()
    with BatchEngine(md_types.init_params(n, L, 0.005, rc), 1) as eng:
        epot0 = eng.prepare(SEED_BASE, target)[0][0]
        assert np.stack([x[0] for x in eng.get_state(("v",))["v"]]).tobytes() == v.tobytes()
    d_epot = abs(epot0 - epot_ref)
    assert d_epot <= 1e-13 * abs(epot_ref)
    bound = (0.5 * d_epot / (target - epot_ref) + n * 2.0 ** -53) * np.abs(v_ref).max()
    dv = np.abs(v - v_ref).max()
    print(f"run_0001: max |dv| = {dv:.3e}, bound {bound:.3e}")
    assert dv <= bound
    assert many[1]["rva.dat"] != many[2]["rva.dat"] != many[3]["rva.dat"] != many[1]["rva.dat"]
    for i in (1, 2, 3):
        one = _run(tmp_path / f"one_{i}", 1, SEED_BASE + i - 1)[1]
        assert set(one) == set(many[i])
        for name in one:
            assert one[name] == many[i][name], (i, name)
