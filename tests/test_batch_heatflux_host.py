"""CPU-only: the heat flux entry points of the batch engine (include/ljmd.h, ljmd_batch_heatflux_*) reject a NULL handle,
the Python BatchEngine checks what it can before it calls the library, the limit is the same in the header, the wrapper
and the kernels' header, the entry points' host code runs on the fake HIP runtime (tests/batch_heatflux_host, a program of
its own under ASan and UBSan), and analysis.heat_flux_acf_ensemble is the plain loop over the replicas."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from ljmd_amd import BatchEngine, PerReplicaBatchEngine, _lib, analysis, md_types, synthetic

CSRC = ROOT / "molecular-dynamics-simulation---lennard-jones-monoatomic-fluid_amd" / "csrc"


def test_heatflux_entry_points_reject_a_null_handle():
    lib = _lib.load()
    assert lib.ljmd_batch_heatflux_configure(None, 16, 0) == _lib.LJMD_ERR_INVALID_ARG
    assert "ljmd_batch_heatflux_configure: NULL handle" in _lib.batch_last_error()
    assert lib.ljmd_batch_heatflux_configure(None, -1, -1) == _lib.LJMD_ERR_INVALID_ARG     # the handle comes first
    assert "NULL handle" in _lib.batch_last_error()
    assert lib.ljmd_batch_heatflux_accumulate(None) == _lib.LJMD_ERR_INVALID_ARG
    assert lib.ljmd_batch_heatflux_read(None, None, None, None) == _lib.LJMD_ERR_INVALID_ARG
    assert lib.ljmd_batch_heatflux_read_exact(None, None, None) == _lib.LJMD_ERR_INVALID_ARG
    assert lib.ljmd_batch_heatflux_reset(None) == _lib.LJMD_ERR_INVALID_ARG
    assert "ljmd_batch_heatflux_reset" in _lib.batch_last_error()


def test_the_limit_is_the_same_everywhere():
    assert _lib.BATCH_HEATFLUX_MAX_SNAPSHOTS == _lib.HEATFLUX_MAX_SNAPSHOTS == 262144
    header = (ROOT / "include" / "ljmd.h").read_text()
    assert re.findall(r"^#define LJMD_BATCH_HEATFLUX_MAX_SNAPSHOTS (\d+)$", header, flags=re.M) == ["262144"]
    kernel_header = (CSRC / "ljmd_batch_heatflux.h").read_text()
    assert re.findall(r"kBatchHeatfluxMaxSnapshots = (\d+);", kernel_header) == ["262144"]
    fortran = (CSRC.parent / "fortran" / "ljmd_c_api.f90").read_text()
    assert re.findall(r"LJMD_BATCH_HEATFLUX_MAX_SNAPSHOTS = (\d+)$", fortran, flags=re.M) == ["262144"]


def _unopened(cls, n_replicas, n):
    """an engine whose handle was never created: the checks below run before any library call"""
    eng = object.__new__(cls)
    eng._lib = _lib.load()
    params = md_types.init_params(n, synthetic.box_length(n), 0.005, 0.49 * synthetic.box_length(n))
    if cls is PerReplicaBatchEngine:
        eng.params_list = [params] * n_replicas
    else:
        eng.params = params
    eng.n_replicas = n_replicas
    eng._h = None
    return eng


@pytest.mark.parametrize("cls", [BatchEngine, PerReplicaBatchEngine])
def test_batch_engine_heatflux_checks_before_the_library(cls):
    eng = _unopened(cls, 4, 108)
    for read in (eng.heatflux_read, eng.heatflux_read_exact):
        with pytest.raises(ValueError, match="heatflux_configure"):
            read()                                           # no series known yet: no shape to return
    for bad in (2.0, "3", None, True, np.float64(4.0)):
        with pytest.raises(TypeError, match="max_snapshots"):
            eng.heatflux_configure(bad)
        with pytest.raises(TypeError, match="every"):
            eng.heatflux_configure(4, every=bad)
    with pytest.raises(ValueError, match="int32"):
        eng.heatflux_configure(2 ** 31)
    with pytest.raises(ValueError, match="int32"):
        eng.heatflux_configure(4, every=-2 ** 31 - 1)
    with pytest.raises(ValueError, match="heatflux_configure"):
        eng.heatflux_read()                                  # a refused configure leaves nothing behind
    # what passes the checks reaches the library, which refuses the handle that was never created
    with pytest.raises(_lib.LjmdError) as ei:
        eng.heatflux_configure(np.int64(8), every=np.int32(2))
    assert ei.value.code == _lib.LJMD_ERR_INVALID_ARG and "ljmd_batch_heatflux_configure" in ei.value.message
    with pytest.raises(ValueError, match="heatflux_configure"):
        eng.heatflux_read_exact()


def test_heat_flux_acf_ensemble_is_the_loop_over_replicas():
    rng = np.random.Generator(np.random.PCG64(17))
    n_snap, B, max_lag = 40, 6, 7
    j = rng.normal(size=(n_snap, B, 3))
    for stride in (1, 3):
        mean, err = analysis.heat_flux_acf_ensemble(j, max_lag, stride)
        want = np.empty((B, max_lag + 1))
        for b in range(B):                                   # replica by replica: J(0) . J(tau) / 3 over the origins
            for lag in range(max_lag + 1):
                # the reference's convention: the last snapshot is no origin, not even of lag 0
                origins = [t0 for t0 in range(0, n_snap - 1, stride) if t0 + lag <= n_snap - 1]
                want[b, lag] = sum(float(np.dot(j[t0, b], j[t0 + lag, b])) for t0 in origins) / len(origins) / 3.0
        assert np.array_equal(np.stack([analysis.heat_flux_acf(j[:, b], max_lag, stride) for b in range(B)]).mean(axis=0), mean)
        # the explicit sums add in another order than the library's: a few ulp of the largest term
        assert np.allclose(mean, want.mean(axis=0), rtol=0.0, atol=1e-13)
        assert np.allclose(err, want.std(axis=0, ddof=1) / np.sqrt(B), rtol=0.0, atol=1e-13)
        assert mean.shape == err.shape == (max_lag + 1,) and np.all(err > 0.0)
    one_mean, one_err = analysis.heat_flux_acf_ensemble(j[:, :1], max_lag)
    assert np.array_equal(one_mean, analysis.heat_flux_acf(j[:, 0], max_lag)) and np.all(np.isnan(one_err))
    for bad in (j[:, 0], j[:, :, :2], j[:, :0]):
        with pytest.raises(ValueError, match="heat_flux_acf_ensemble"):
            analysis.heat_flux_acf_ensemble(bad)


def test_heatflux_host_code_under_sanitizers():
    """guard order, the unchanged launches of a handle without the feature, rows / chunks / streams of the snapshots inside
    steps beside the pressure tensor, the full-series refusal, poison without a counted snapshot, allocations freed: the
    program checks itself"""
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc absent: the program cannot be built")
    here = ROOT / "tests" / "batch_heatflux_host"
    subprocess.run(["make", "-C", str(here)], check=True, capture_output=True, timeout=600)
    env = {k: v for k, v in os.environ.items() if not k.startswith("LJMD_")}
    env.update(FAKEHIP_DEVICES="1", ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:exitcode=23",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1:exitcode=24")
    out = subprocess.run([str(here / "batch_heatflux_host")], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-6000:])
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error:" not in out.stderr, out.stderr[-6000:]
    assert out.stdout.strip().splitlines()[-1] == "batch_heatflux_host: ok" and "FAILED" not in out.stdout
