"""CPU-only: the host core of the engine's resident g(r) (csrc/ljmd_rdf.cpp) on the fake HIP runtime, and the tile-pair
bound its kernel skips by (csrc/ljmd_rdf.h).  tests/rdf_host is a program of its own under ASan and UBSan that checks
itself: every guard with its return code and message, the configure / accumulate / read / reset sequences, the bound
that keeps a 32-bit LDS bin from overflowing for n up to 2^23, and rdf_tile_gap2 against brute force over sample points
of random and adversarial boxes.  The entry points themselves are covered on the GPU (tests/test_gpu_rdf_resident.py);
here only that they exist and refuse a NULL handle."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT
from ljmd_amd import Engine, _lib


def test_rdf_host_code_under_sanitizers():
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc absent: the program cannot be built")
    here = ROOT / "tests" / "rdf_host"
    subprocess.run(["make", "-C", str(here)], check=True, capture_output=True, timeout=600)
    env = {k: v for k, v in os.environ.items() if not k.startswith("LJMD_")}
    env.update(FAKEHIP_DEVICES="1", ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:exitcode=23",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1:exitcode=24")
    out = subprocess.run([str(here / "rdf_host")], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-6000:])
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error:" not in out.stderr, out.stderr[-6000:]
    assert out.stdout.strip().splitlines()[-1] == "rdf_host: ok" and "FAILED" not in out.stdout


def test_entry_points_refuse_a_null_handle():
    lib = _lib.load()
    assert lib.ljmd_rdf_configure(None, 10, 1.0) == _lib.LJMD_ERR_INVALID_ARG
    assert "ljmd_rdf_configure" in _lib.last_error()
    assert lib.ljmd_rdf_accumulate(None) == _lib.LJMD_ERR_INVALID_ARG
    assert lib.ljmd_rdf_read(None, None, None) == _lib.LJMD_ERR_INVALID_ARG
    assert lib.ljmd_rdf_reset(None) == _lib.LJMD_ERR_INVALID_ARG
    assert lib.ljmd_rdf_profile_read(None, None, None, None) == _lib.LJMD_ERR_INVALID_ARG
    for name in ("rdf_configure", "rdf_accumulate", "rdf_read", "rdf_reset", "rdf_profile"):
        assert callable(getattr(Engine, name))
