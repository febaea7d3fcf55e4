"""-m gpu: bin/md_simulation_many_gpu with LJMD_HEATFLUX=1 -- the heat flux of every run recorded on the device
(ljmd_batch_heatflux_*) at the sampling instants that write rva.dat.  Two runs at N = 108 (k = 3), 300 steps, prepared on
the device (LJMD_SEED_BASE): outputs/run_NNNN/heat_flux_gpu.dat has one line per sampling instant, its rows are the CPU
model (tests/heatflux_model.py) on the run's own rva.dat bit for bit, in the reproducible mode the file is byte for byte
what md_simulation_gpu writes for that run, heat_flux_acf_gpu.dat appears only with LJMD_HEATFLUX_MAX_LAG > 0, and every
other output file does not notice the variables."""
import numpy as np
import pytest

import heatflux_model
from ljmd_amd import io_formats
from test_gpu_batch_stress_fortran import L, RC_OVER_L, RUNS, SAMPLES, _many, _one

pytestmark = pytest.mark.gpu

HEADER = "# time   J_x   J_y   J_z   conv_x   conv_y   conv_z   pot_x   pot_y   pot_z   coll_x   coll_y   coll_z"


def _rows(flux):
    lines = flux.decode().splitlines()
    assert lines[0] == HEADER
    rows = np.array([[float(x) for x in ln.split()] for ln in lines[1:]])
    assert rows.shape == (SAMPLES, 13)                        # one line per sampling instant
    return rows


def test_run_many_driver_writes_the_heat_flux_of_every_run(tmp_path):
    repro = dict(LJMD_REPRODUCIBLE="1")
    plain = _many(tmp_path / "unset", **repro)
    only = _many(tmp_path / "flux", LJMD_HEATFLUX="1", **repro)
    on = _many(tmp_path / "on", LJMD_HEATFLUX="1", LJMD_HEATFLUX_MAX_LAG="3", **repro)
    off = _many(tmp_path / "zero", LJMD_HEATFLUX="0", LJMD_HEATFLUX_MAX_LAG="3", **repro)
    assert off == plain
    fluxes = {}
    for i in range(1, RUNS + 1):
        assert "rva.dat" in plain[i] and "md_final_results.txt" in plain[i] and "rv_init_gpu.dat" in plain[i]
        assert "heat_flux_gpu.dat" not in plain[i] and "heat_flux_acf_gpu.dat" not in plain[i]
        fluxes[i] = only[i].pop("heat_flux_gpu.dat")
        assert only[i] == plain[i]                            # no ACF file without a lag, every other file byte for byte
        flux, acf = on[i].pop("heat_flux_gpu.dat"), on[i].pop("heat_flux_acf_gpu.dat")
        assert on[i] == plain[i] and flux == fluxes[i]
        alines = acf.decode().splitlines()
        assert alines[0] == "# lag   tau   ACF_J   lambda" and len(alines) == 1 + 4

        # one line per sampling instant, each the model's doubles for that record of the run's own rva.dat
        rows = _rows(fluxes[i])
        head, snaps = io_formats.read_rva(tmp_path / "flux" / "outputs" / f"run_{i:04d}" / "rva.dat")
        assert snaps.shape[0] == SAMPLES and snaps.shape[3] == 108
        np.testing.assert_allclose(rows[:, 0], (np.arange(SAMPLES) + 2) * 50 * 5e-3, rtol=1e-12)
        for s in range(SAMPLES):
            w, flag = heatflux_model.words(snaps[s, 0], snaps[s, 2], L, RC_OVER_L * L)
            assert not flag
            j, parts = heatflux_model.doubles(w, L)
            assert rows[s, 1:4].tobytes() == j.tobytes(), (i, s)
            assert rows[s, 4:].tobytes() == parts.tobytes(), (i, s)
    assert fluxes[1] != fluxes[2]                             # independent runs

    # reproducible mode: the heat flux file of a run is what md_simulation_gpu writes for that run
    for i in range(1, RUNS + 1):
        rv = tmp_path / "flux" / "outputs" / f"run_{i:04d}" / "rv_init_gpu.dat"
        one = _one(tmp_path / f"one_{i}", rv, LJMD_HEATFLUX="1", **repro)
        assert one["heat_flux_gpu.dat"] == fluxes[i], i
        assert one["rva.dat"] == plain[i]["rva.dat"]


def test_fp64_mode_leaves_every_other_file_alone(tmp_path):
    plain = _many(tmp_path / "unset")
    on = _many(tmp_path / "on", LJMD_HEATFLUX="1")
    zero = _many(tmp_path / "zero", LJMD_HEATFLUX="0")
    assert zero == plain
    for i in range(1, RUNS + 1):
        rows = _rows(on[i].pop("heat_flux_gpu.dat"))
        assert on[i] == plain[i]
        assert np.isfinite(rows).all() and np.abs(rows[:, 1:]).min() > 0.0
