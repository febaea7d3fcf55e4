"""CPU-only: the host core of the engine's resident MSD / VACF (csrc/ljmd_tcf.cpp) on the fake HIP runtime.
tests/tcf_host is a program of its own under ASan and UBSan that checks itself: its launchers carry out the kernels'
meaning on the host, and the words the core returns must equal a brute-force sum over the stored snapshots -- several
(max_lag, stride) pairs, a slot permutation that changes between snapshots, ring wrap, a new trajectory -- with every
guard's return code and message, the arguments of every launch and the byte counts of configure for n up to 2^23.  The
entry points themselves are covered on the GPU (tests/test_gpu_tcf_resident.py); here that they exist and refuse a NULL
handle, the checks Engine makes before it calls the library, and the two limits in the three places that state them."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT
from ljmd_amd import Engine, _lib, md_types, synthetic

PKG = ROOT / "molecular-dynamics-simulation---lennard-jones-monoatomic-fluid_amd"


def test_tcf_host_code_under_sanitizers():
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc absent: the program cannot be built")
    here = ROOT / "tests" / "tcf_host"
    subprocess.run(["make", "-C", str(here)], check=True, capture_output=True, timeout=600)
    env = {k: v for k, v in os.environ.items() if not k.startswith("LJMD_")}
    env.update(FAKEHIP_DEVICES="1", ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:exitcode=23",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1:exitcode=24")
    out = subprocess.run([str(here / "tcf_host")], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-6000:])
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error:" not in out.stderr, out.stderr[-6000:]
    assert out.stdout.strip().splitlines()[-1] == "tcf_host: ok" and "FAILED" not in out.stdout


def test_entry_points_refuse_a_null_handle():
    lib = _lib.load()
    assert lib.ljmd_tcf_configure(None, 10, 1) == _lib.LJMD_ERR_INVALID_ARG
    assert "ljmd_tcf_configure" in _lib.last_error()
    assert lib.ljmd_tcf_accumulate(None) == _lib.LJMD_ERR_INVALID_ARG
    assert "ljmd_tcf_accumulate" in _lib.last_error()
    assert lib.ljmd_tcf_read(None, None, None, None, None) == _lib.LJMD_ERR_INVALID_ARG
    assert "ljmd_tcf_read" in _lib.last_error()
    assert lib.ljmd_tcf_read_exact(None, None, None, None) == _lib.LJMD_ERR_INVALID_ARG
    assert "ljmd_tcf_read_exact" in _lib.last_error()
    assert lib.ljmd_tcf_reset(None) == _lib.LJMD_ERR_INVALID_ARG
    assert "ljmd_tcf_reset" in _lib.last_error()
    assert lib.ljmd_tcf_profile_read(None, None, None) == _lib.LJMD_ERR_INVALID_ARG
    assert "ljmd_tcf_profile_read" in _lib.last_error()
    for name in ("tcf_configure", "tcf_accumulate", "tcf_read", "tcf_read_exact", "tcf_reset", "tcf_profile"):
        assert callable(getattr(Engine, name))


def _unopened(n):
    """an Engine whose handle was never created: the checks below run before any library call"""
    eng = object.__new__(Engine)
    eng._lib = _lib.load()
    eng.params = md_types.init_params(n, synthetic.box_length(n), 0.005, 0.49 * synthetic.box_length(n))
    eng._h = None
    return eng


def test_engine_tcf_checks_before_the_library():
    eng = _unopened(108)
    with pytest.raises(ValueError, match="tcf_configure"):
        eng.tcf_read()                                       # no max_lag known yet: no shape to return
    with pytest.raises(ValueError, match="tcf_configure"):
        eng.tcf_read_exact()
    for bad in (2.5, "4", None, True, [4]):
        with pytest.raises(TypeError, match="max_lag"):
            eng.tcf_configure(bad)
        with pytest.raises(TypeError, match="origin_stride"):
            eng.tcf_configure(4, origin_stride=bad)
    with pytest.raises(ValueError, match="tcf_configure"):
        eng.tcf_read()                                       # a refused configure leaves nothing behind


def test_limits_agree_between_header_python_and_fortran():
    header = (ROOT / "include" / "ljmd.h").read_text()
    fortran = (PKG / "fortran" / "ljmd_c_api.f90").read_text()
    for name, value in (("LJMD_TCF_MAX_LAG", _lib.TCF_MAX_LAG), ("LJMD_TCF_MAX_ORIGINS", _lib.TCF_MAX_ORIGINS)):
        in_header = re.findall(rf"^#define {name} (\d+)$", header, flags=re.M)
        in_fortran = re.findall(rf"parameter(?:\s*,\s*public)?\s*::\s*{name}\s*=\s*(\d+)", fortran, flags=re.I)
        assert in_header == [str(value)], (name, in_header)
        assert in_fortran == [str(value)], (name, in_fortran)
    assert (_lib.TCF_MAX_LAG, _lib.TCF_MAX_ORIGINS) == (_lib.BATCH_TCF_MAX_LAG, _lib.BATCH_TCF_MAX_ORIGINS)
