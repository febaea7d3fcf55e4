"""CPU-only: the host core of the engine's resident van Hove self-correlation (csrc/ljmd_vanhove.cpp) on the fake HIP
runtime.  tests/vanhove_host is a program of its own under ASan and UBSan that checks itself: its launchers carry out
the kernels' meaning on the host, and the counts and words the core returns must equal a brute-force loop over the
stored snapshots -- several (max_lag, stride, nbins), a slot permutation that changes between snapshots, ring wrap, a
new trajectory, chunk overrides -- with every guard's return code and message in order, the arguments of every launch,
the byte counts of configure for n up to 2^23 and the refusal of rank and multi views.  The entry points themselves are
covered on the GPU (tests/test_gpu_vanhove_resident.py); here that they exist and refuse a NULL handle, the checks Engine
makes before it calls the library, and the three limits in the three places that state them."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT
from ljmd_amd import Engine, _lib, md_types, synthetic

PKG = ROOT / "molecular-dynamics-simulation---lennard-jones-monoatomic-fluid_amd"


def test_vanhove_host_code_under_sanitizers():
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc absent: the program cannot be built")
    here = ROOT / "tests" / "vanhove_host"
    subprocess.run(["make", "-C", str(here)], check=True, capture_output=True, timeout=600)
    env = {k: v for k, v in os.environ.items() if not k.startswith("LJMD_")}
    env.update(FAKEHIP_DEVICES="1", ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:exitcode=23",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1:exitcode=24")
    out = subprocess.run([str(here / "vanhove_host")], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-6000:])
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error:" not in out.stderr, out.stderr[-6000:]
    assert out.stdout.strip().splitlines()[-1] == "vanhove_host: ok" and "FAILED" not in out.stdout


def test_entry_points_refuse_a_null_handle():
    lib = _lib.load()
    assert lib.ljmd_vanhove_configure(None, 10, 1, 64, 1.0) == _lib.LJMD_ERR_INVALID_ARG
    assert "ljmd_vanhove_configure" in _lib.last_error()
    assert lib.ljmd_vanhove_accumulate(None) == _lib.LJMD_ERR_INVALID_ARG
    assert "ljmd_vanhove_accumulate" in _lib.last_error()
    assert lib.ljmd_vanhove_read(None, None, None, None, None, None) == _lib.LJMD_ERR_INVALID_ARG
    assert "ljmd_vanhove_read" in _lib.last_error()
    assert lib.ljmd_vanhove_read_exact(None, None, None, None, None) == _lib.LJMD_ERR_INVALID_ARG
    assert "ljmd_vanhove_read_exact" in _lib.last_error()
    assert lib.ljmd_vanhove_reset(None) == _lib.LJMD_ERR_INVALID_ARG
    assert "ljmd_vanhove_reset" in _lib.last_error()
    assert lib.ljmd_vanhove_profile_read(None, None, None) == _lib.LJMD_ERR_INVALID_ARG
    assert "ljmd_vanhove_profile_read" in _lib.last_error()
    for name in ("vanhove_configure", "vanhove_accumulate", "vanhove_read", "vanhove_read_exact", "vanhove_reset",
                 "vanhove_profile"):
        assert callable(getattr(Engine, name))


def _unopened(n):
    """an Engine whose handle was never created: the checks below run before any library call"""
    eng = object.__new__(Engine)
    eng._lib = _lib.load()
    eng.params = md_types.init_params(n, synthetic.box_length(n), 0.005, 0.49 * synthetic.box_length(n))
    eng._h = None
    return eng


def test_engine_vanhove_checks_before_the_library():
    eng = _unopened(108)
    with pytest.raises(ValueError, match="vanhove_configure"):
        eng.vanhove_read()                                   # no shape known yet: nothing to return
    with pytest.raises(ValueError, match="vanhove_configure"):
        eng.vanhove_read_exact()
    for bad in (2.5, "4", None, True, [4]):
        with pytest.raises(TypeError, match="max_lag"):
            eng.vanhove_configure(bad)
        with pytest.raises(TypeError, match="origin_stride"):
            eng.vanhove_configure(4, origin_stride=bad)
        with pytest.raises(TypeError, match="nbins"):
            eng.vanhove_configure(4, 1, nbins=bad)
    for bad in ("1.0", True, [1.0]):
        with pytest.raises(TypeError, match="rmax"):
            eng.vanhove_configure(4, 1, 64, rmax=bad)
    with pytest.raises(ValueError, match="vanhove_configure"):
        eng.vanhove_read()                                   # a refused configure leaves nothing behind


def test_limits_agree_between_header_python_and_fortran():
    header = (ROOT / "include" / "ljmd.h").read_text()
    fortran = (PKG / "fortran" / "ljmd_c_api.f90").read_text()
    for name, value in (("LJMD_VANHOVE_MAX_LAG", _lib.VANHOVE_MAX_LAG), ("LJMD_VANHOVE_MAX_ORIGINS", _lib.VANHOVE_MAX_ORIGINS),
                        ("LJMD_VANHOVE_MAX_BINS", _lib.VANHOVE_MAX_BINS)):
        in_header = re.findall(rf"^#define {name} (\d+)$", header, flags=re.M)
        in_fortran = re.findall(rf"parameter(?:\s*,\s*public)?\s*::\s*{name}\s*=\s*(\d+)", fortran, flags=re.I)
        assert in_header == [str(value)], (name, in_header)
        assert in_fortran == [str(value)], (name, in_fortran)
    assert (_lib.VANHOVE_MAX_LAG, _lib.VANHOVE_MAX_ORIGINS) == (_lib.TCF_MAX_LAG, _lib.TCF_MAX_ORIGINS)
    assert (_lib.VANHOVE_MAX_LAG, _lib.VANHOVE_MAX_ORIGINS, _lib.VANHOVE_MAX_BINS) == (4096, 512, 4096)
