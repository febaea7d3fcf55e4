"""CPU-only: the van Hove entry points of the batch engine (include/ljmd.h, ljmd_batch_vanhove_*) reject a NULL handle,
the Python BatchEngine checks what it can before it calls the library, the limits are the same in the header, the wrapper,
the kernels' header and the Fortran binding, the entry points' host code runs on the fake HIP runtime against a
brute-force loop (tests/batch_vanhove_host, a program of its own under ASan and UBSan), and
analysis.van_hove_self_ensemble is the plain numpy mean and standard error over the replicas."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from ljmd_amd import BatchEngine, PerReplicaBatchEngine, _lib, analysis
from test_batch_heatflux_host import _unopened

CSRC = ROOT / "molecular-dynamics-simulation---lennard-jones-monoatomic-fluid_amd" / "csrc"


def test_vanhove_entry_points_reject_a_null_handle():
    lib = _lib.load()
    assert lib.ljmd_batch_vanhove_configure(None, 8, 1, 16, None, 0) == _lib.LJMD_ERR_INVALID_ARG
    assert "ljmd_batch_vanhove_configure: NULL handle" in _lib.batch_last_error()
    assert lib.ljmd_batch_vanhove_configure(None, -1, 0, 0, None, -1) == _lib.LJMD_ERR_INVALID_ARG     # the handle comes first
    assert "NULL handle" in _lib.batch_last_error()
    assert lib.ljmd_batch_vanhove_accumulate(None) == _lib.LJMD_ERR_INVALID_ARG
    assert lib.ljmd_batch_vanhove_read(None, None, None, None, None, None) == _lib.LJMD_ERR_INVALID_ARG
    assert lib.ljmd_batch_vanhove_read_exact(None, None, None, None, None) == _lib.LJMD_ERR_INVALID_ARG
    assert lib.ljmd_batch_vanhove_reset(None) == _lib.LJMD_ERR_INVALID_ARG
    assert "ljmd_batch_vanhove_reset" in _lib.batch_last_error()


def test_the_limits_are_the_same_everywhere():
    want = {"MAX_LAG": 4096, "MAX_ORIGINS": 512, "MAX_BINS": 1024}
    header = (ROOT / "include" / "ljmd.h").read_text()
    kernel_header = (CSRC / "ljmd_batch_vanhove.h").read_text()
    fortran = (CSRC.parent / "fortran" / "ljmd_c_api.f90").read_text()
    for name, value in want.items():
        assert getattr(_lib, f"BATCH_VANHOVE_{name}") == value
        assert re.findall(rf"^#define LJMD_BATCH_VANHOVE_{name} (\d+)$", header, flags=re.M) == [str(value)]
        camel = "".join(w.capitalize() for w in name.split("_"))
        assert re.findall(rf"kBatchVanhove{camel} = (\d+);", kernel_header) == [str(value)]
        assert re.findall(rf"LJMD_BATCH_VANHOVE_{name} = (\d+)$", fortran, flags=re.M) == [str(value)]
    # the batch bin cap is what the LDS budget of the kernel leaves: 513 entries of 32 bytes and 1025 bins of 4
    assert 513 * 32 + 1025 * 4 == 20516 <= 24 * 1024


@pytest.mark.parametrize("cls", [BatchEngine, PerReplicaBatchEngine])
def test_batch_engine_vanhove_checks_before_the_library(cls):
    eng = _unopened(cls, 4, 108)
    for read in (eng.vanhove_read, eng.vanhove_read_exact):
        with pytest.raises(ValueError, match="vanhove_configure"):
            read()                                           # no shape known yet
    for bad in (2.0, "3", None, True, np.float64(4.0)):
        with pytest.raises(TypeError, match="max_lag"):
            eng.vanhove_configure(bad)
        with pytest.raises(TypeError, match="origin_stride"):
            eng.vanhove_configure(4, bad)
        with pytest.raises(TypeError, match="nbins"):
            eng.vanhove_configure(4, 1, bad)
        with pytest.raises(TypeError, match="every"):
            eng.vanhove_configure(4, every=bad)
    with pytest.raises(ValueError, match="int32"):
        eng.vanhove_configure(2 ** 31)
    with pytest.raises(ValueError, match="int32"):
        eng.vanhove_configure(4, every=-2 ** 31 - 1)
    for bad in ("1.0", True, [True] * 4, 1j):
        with pytest.raises(TypeError, match="rmax"):
            eng.vanhove_configure(4, rmax=bad)
    for bad in ([1.0, 2.0], np.ones((4, 1)), np.ones(5)):
        with pytest.raises(ValueError, match="rmax"):
            eng.vanhove_configure(4, rmax=bad)
    with pytest.raises(ValueError, match="vanhove_configure"):
        eng.vanhove_read()                                   # a refused configure leaves nothing behind
    # what passes the checks reaches the library, which refuses the handle that was never created
    for rmax in (None, 2, 1.5, np.float32(1.5), [1.0, 2.0, 3.0, 4.0], np.arange(1, 5)):
        with pytest.raises(_lib.LjmdError) as ei:
            eng.vanhove_configure(np.int64(8), np.int32(2), 16, rmax, every=np.int32(2))
        assert ei.value.code == _lib.LJMD_ERR_INVALID_ARG and "ljmd_batch_vanhove_configure" in ei.value.message
    with pytest.raises(ValueError, match="vanhove_configure"):
        eng.vanhove_read_exact()


def test_van_hove_self_ensemble_is_the_mean_and_standard_error_over_replicas():
    rng = np.random.Generator(np.random.PCG64(23))
    B, rows, nbins, n, dr = 6, 5, 12, 108, 0.01
    counts = np.array([4, 4, 3, 2, 0], dtype=np.int64)
    hist = np.zeros((B, rows, nbins + 1), dtype=np.uint64)
    for b in range(B):
        for l in range(rows):
            hist[b, l] = rng.multinomial(n * int(counts[l]), np.full(nbins + 1, 1.0 / (nbins + 1)))
    r, mean, err, overflow = analysis.van_hove_self_ensemble(hist, counts, n, dr)
    per = [analysis.van_hove_self(hist[b], counts, n, dr) for b in range(B)]
    g = np.stack([p[1] for p in per])
    assert np.array_equal(r, per[0][0]) and mean.shape == err.shape == (rows, nbins)
    assert np.array_equal(mean, g.mean(axis=0)) and np.array_equal(err, g.std(axis=0, ddof=1) / np.sqrt(B))
    assert np.array_equal(overflow, np.stack([p[2] for p in per]).mean(axis=0))
    # by hand: H / (n count V_shell), averaged
    b_ = np.arange(nbins)
    shell = 4.0 * np.pi / 3.0 * ((b_ + 1.0) ** 3 - b_ ** 3) * dr ** 3
    want = hist[:, :4, :-1].astype(np.float64) / (n * counts[:4, None] * shell[None, :])
    assert np.allclose(mean[:4], want.mean(axis=0), rtol=1e-14, atol=0.0)
    assert np.allclose(err[:4], want.std(axis=0, ddof=1) / np.sqrt(B), rtol=1e-12, atol=0.0)
    assert np.all(err[:4] > 0.0) and not mean[4].any() and not err[4].any()       # a lag without origins is 0
    assert np.allclose((mean[:4] * shell).sum(axis=1) + overflow[:4], 1.0, rtol=0.0, atol=1e-14)
    _, one_mean, one_err, _ = analysis.van_hove_self_ensemble(hist[:1], counts, n, dr)
    assert np.array_equal(one_mean, per[0][1]) and np.all(np.isnan(one_err))
    for bad in (hist[0], hist[:0], hist[..., None]):
        with pytest.raises(ValueError, match="van_hove_self_ensemble"):
            analysis.van_hove_self_ensemble(bad, counts, n, dr)


def test_vanhove_host_code_under_sanitizers():
    """the C ABI against a brute-force loop over stored snapshots -- several shapes, per-replica n and rmax, ring wrap, a
    new trajectory, `every` inside steps -- every guard's code and message, the arguments of every launch, the byte counts
    of configure, the range word, poison and recovery, allocations freed: the program checks itself"""
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc absent: the program cannot be built")
    here = ROOT / "tests" / "batch_vanhove_host"
    subprocess.run(["make", "-C", str(here)], check=True, capture_output=True, timeout=600)
    env = {k: v for k, v in os.environ.items() if not k.startswith("LJMD_")}
    env.update(FAKEHIP_DEVICES="1", ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:exitcode=23",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1:exitcode=24")
    out = subprocess.run([str(here / "batch_vanhove_host")], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-6000:])
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error:" not in out.stderr, out.stderr[-6000:]
    assert out.stdout.strip().splitlines()[-1] == "batch_vanhove_host: ok" and "FAILED" not in out.stdout
