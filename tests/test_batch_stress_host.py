"""CPU-only: the pressure tensor entry points of the batch engine (include/ljmd.h, ljmd_batch_stress_*) reject a NULL
handle, the Python BatchEngine checks what it can before it calls the library, the limit is the same in the header, the
wrapper and the kernels' header, and the entry points' host code runs on the fake HIP runtime (tests/batch_stress_host, a
program of its own under ASan and UBSan)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from ljmd_amd import BatchEngine, _lib, md_types, synthetic

CSRC = ROOT / "molecular-dynamics-simulation---lennard-jones-monoatomic-fluid_amd" / "csrc"


def test_stress_entry_points_reject_a_null_handle():
    lib = _lib.load()
    assert lib.ljmd_batch_stress_configure(None, 16, 0) == _lib.LJMD_ERR_INVALID_ARG
    assert "ljmd_batch_stress_configure: NULL handle" in _lib.batch_last_error()
    assert lib.ljmd_batch_stress_configure(None, -1, -1) == _lib.LJMD_ERR_INVALID_ARG     # the handle comes first
    assert "NULL handle" in _lib.batch_last_error()
    assert lib.ljmd_batch_stress_accumulate(None) == _lib.LJMD_ERR_INVALID_ARG
    assert lib.ljmd_batch_stress_read(None, None, None) == _lib.LJMD_ERR_INVALID_ARG
    assert lib.ljmd_batch_stress_read_exact(None, None, None) == _lib.LJMD_ERR_INVALID_ARG
    assert lib.ljmd_batch_stress_reset(None) == _lib.LJMD_ERR_INVALID_ARG
    assert "ljmd_batch_stress_reset" in _lib.batch_last_error()


def test_the_limit_is_the_same_everywhere():
    assert _lib.BATCH_STRESS_MAX_SNAPSHOTS == _lib.STRESS_MAX_SNAPSHOTS == 262144
    header = (ROOT / "include" / "ljmd.h").read_text()
    assert re.findall(r"^#define LJMD_BATCH_STRESS_MAX_SNAPSHOTS (\d+)$", header, flags=re.M) == ["262144"]
    kernel_header = (CSRC / "ljmd_batch_stress.h").read_text()
    assert re.findall(r"kBatchStressMaxSnapshots = (\d+);", kernel_header) == ["262144"]


def _unopened(n_replicas, n):
    """a BatchEngine whose handle was never created: the checks below run before any library call"""
    eng = object.__new__(BatchEngine)
    eng._lib = _lib.load()
    eng.params = md_types.init_params(n, synthetic.box_length(n), 0.005, 0.49 * synthetic.box_length(n))
    eng.n_replicas = n_replicas
    eng._h = None
    return eng


def test_batch_engine_stress_checks_before_the_library():
    eng = _unopened(4, 108)
    for read in (eng.stress_read, eng.stress_read_exact):
        with pytest.raises(ValueError, match="stress_configure"):
            read()                                           # no series known yet: no shape to return
    for bad in (2.0, "3", None, True, np.float64(4.0)):
        with pytest.raises(TypeError, match="max_snapshots"):
            eng.stress_configure(bad)
        with pytest.raises(TypeError, match="every"):
            eng.stress_configure(4, every=bad)
    with pytest.raises(ValueError, match="int32"):
        eng.stress_configure(2 ** 31)
    with pytest.raises(ValueError, match="int32"):
        eng.stress_configure(4, every=-2 ** 31 - 1)
    with pytest.raises(ValueError, match="stress_configure"):
        eng.stress_read()                                    # a refused configure leaves nothing behind
    # what passes the checks reaches the library, which refuses the handle that was never created
    with pytest.raises(_lib.LjmdError) as ei:
        eng.stress_configure(np.int64(8), every=np.int32(2))
    assert ei.value.code == _lib.LJMD_ERR_INVALID_ARG and "ljmd_batch_stress_configure" in ei.value.message
    with pytest.raises(ValueError, match="stress_configure"):
        eng.stress_read_exact()


def test_stress_host_code_under_sanitizers():
    """guard order, the unchanged launches of a handle without the feature, rows / chunks / streams of the snapshots inside
    steps, the full-series refusal, poison without a counted snapshot, allocations freed: the program checks itself"""
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc absent: the program cannot be built")
    here = ROOT / "tests" / "batch_stress_host"
    subprocess.run(["make", "-C", str(here)], check=True, capture_output=True, timeout=600)
    env = {k: v for k, v in os.environ.items() if not k.startswith("LJMD_")}
    env.update(FAKEHIP_DEVICES="1", ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:exitcode=23",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1:exitcode=24")
    out = subprocess.run([str(here / "batch_stress_host")], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-6000:])
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error:" not in out.stderr, out.stderr[-6000:]
    assert out.stdout.strip().splitlines()[-1] == "batch_stress_host: ok" and "FAILED" not in out.stdout
