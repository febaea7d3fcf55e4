"""-m gpu: bin/md_simulation_many_gpu with LJMD_REPRODUCIBLE=1 -- its batch handle in the reproducible mode -- against
bin/md_simulation_gpu with LJMD_REPRODUCIBLE=1, run by run.  The setup of tests/test_gpu_batch_fortran.py: three runs at
N = 108, runs 1 and 3 from their own rv_init.dat, run 2 from the shared one.  In this mode a run's results are a
function of its particles alone, so every output file that both drivers write must be byte for byte equal.  None of
these files carries wall-clock time (both drivers print their rate to stdout only), so no line is left out."""
import os
import shutil
import subprocess

import pytest

from conftest import GOLDEN, ROOT
from ljmd_amd import io_formats, synthetic

pytestmark = pytest.mark.gpu

PKG = ROOT / "molecular-dynamics-simulation---lennard-jones-monoatomic-fluid_amd"
SRC = GOLDEN / "ref_run_n108_oi10"          # N = 108, 1000 steps, output_interval 10, warm-up 100: 90 samples
ENV = dict(os.environ, LJMD_REPRODUCIBLE="1")


def _single_run(workdir, rv_init):
    (workdir / "inputs").mkdir(parents=True)
    (workdir / "outputs" / "one_run").mkdir(parents=True)
    shutil.copy(SRC / "input_simulation_parameters.txt", workdir / "inputs")
    shutil.copy(rv_init, workdir / "outputs" / "rv_init.dat")
    subprocess.run([str(PKG / "bin" / "md_simulation_gpu")], cwd=workdir, check=True, timeout=120, env=ENV)
    return workdir / "outputs" / "one_run"


def test_reproducible_run_many_driver_equals_the_single_run_driver_byte_for_byte(tmp_path):
    exe = PKG / "bin" / "md_simulation_many_gpu"
    assert exe.exists(), "run __graft_entry__.build() first"
    many = tmp_path / "many"
    (many / "inputs").mkdir(parents=True)
    shutil.copy(SRC / "input_simulation_parameters.txt", many / "inputs")
    (many / "outputs").mkdir()
    shutil.copy(SRC / "rv_init.dat", many / "outputs" / "rv_init.dat")
    for run, seed in ((1, 11), (3, 13)):
        p, r, v = synthetic.make_config(108, seed=seed)
        d = many / "outputs" / f"run_{run:04d}"
        d.mkdir()
        io_formats.write_rv_init(d / "rv_init.dat", r[0], r[1], r[2], v[0], v[1], v[2])
    out = subprocess.run([str(exe)], cwd=many, check=True, capture_output=True, text=True, timeout=300,
                         env=dict(ENV, LJMD_RUNS="3"))
    assert "run-steps/s" in out.stdout

    inits = {1: many / "outputs" / "run_0001" / "rv_init.dat", 2: SRC / "rv_init.dat",
             3: many / "outputs" / "run_0003" / "rv_init.dat"}
    for run, rv_init in inits.items():
        mine = many / "outputs" / f"run_{run:04d}"
        single = _single_run(tmp_path / f"single_{run}", rv_init)
        written = sorted(f.name for f in single.iterdir() if f.is_file())
        both = [name for name in written if (mine / name).is_file()]
        # everything the single-run driver writes, the run-many driver writes too
        assert both == written, (run, written, both)
        for name in ("instantaneous_energies.dat", "rva.dat", "md_final_results.txt"):
            assert name in both, (run, name)
        assert sum(name.startswith("corr") for name in both) >= 2, (run, both)
        for name in both:
            assert (mine / name).read_bytes() == (single / name).read_bytes(), (run, name)
