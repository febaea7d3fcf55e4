"""CPU-only: the initial configurations the batch engine prepares on the device (include/ljmd.h, ljmd_batch_prepare).
The definition's CPU model (tests/prepare_model.py) against the reference's own generator output and rv_init.dat, the
entry point's NULL-handle guard, the checks BatchEngine.prepare makes before it calls the library, and the entry
point's host code on the fake HIP runtime (tests/prepare_host, a program of its own under ASan and UBSan)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import prepare_model as P
from conftest import GOLDEN, ROOT
from ljmd_amd import BatchEngine, _lib, io_formats, md_types, synthetic
from reproducible_model import kinetic

# name -> n, L, rc, target_total_energy of the golden inputs (tests/golden/init_k*_warm0/input_simulation_parameters.txt)
GOLDEN_INPUTS = {
    "init_k3_warm0": (108, 5.129927840030091, 0.49 * 5.129927840030091, -500.0),
    "init_k4_warm0": (256, 6.5, 0.35 * 6.5, -900.0),
}


def test_model_ran3_equals_the_reference_module_bit_for_bit():
    ref = np.load(GOLDEN / "ran3_seed-12345_10000.npy")
    mine = P.ran3(-12345, 10000)
    assert mine.shape == ref.shape == (10000,)
    assert np.array_equal(mine.view(np.uint64), ref.view(np.uint64))
    m = P.ran3_states(-12345, 10000)
    assert m.min() >= 0 and m.max() < P.MODULUS


def test_seed_classes_documented_in_the_header():
    """the stream depends on | 1618033 - |seed| | mod 4e6 alone"""
    assert np.array_equal(P.ran3_states(5, 3000), P.ran3_states(-5, 3000))
    assert np.array_equal(P.ran3_states(1618032, 3000), P.ran3_states(1618034, 3000))     # s and 3236066 - s
    assert np.array_equal(P.ran3_states(12345, 3000), P.ran3_states(3236066 - 12345, 3000))
    assert not np.array_equal(P.ran3_states(5, 3000), P.ran3_states(6, 3000))


@pytest.mark.parametrize("name", sorted(GOLDEN_INPUTS))
def test_model_reproduces_the_reference_rv_init(name):
    n, L, _rc, target = GOLDEN_INPUTS[name]
    r_ref, v_ref = io_formats.read_rv_init(GOLDEN / name / "rv_init.dat", n)
    epot_ref = float(np.fromfile(GOLDEN / name / "epot.bin", dtype=np.float64)[0])
    assert np.array_equal(P.lattice(n, L).view(np.uint64), r_ref.view(np.uint64))
    v0 = P.velocities(n, 12345)
    v = v0 * P.scale_factor(target, epot_ref, kinetic(v0))
    err = np.abs(v - v_ref).max() / np.abs(v_ref).max()
    print(f"{name}: max |dv| / max |v| = {err:.3e}")
    # the worst-case error of the reference's own sequential sums (centre of mass, kinetic energy) of n terms
    assert err <= n * 2.0 ** -53


def test_model_removes_the_centre_of_mass():
    v = P.velocities(108, 7)
    assert np.abs(v.sum(axis=1)).max() < 108 * 2.0 ** -52
    assert np.abs(v).max() < 1.0                      # |draw - 0.5| <= 0.5 and |v_cm| <= 0.5
    with pytest.raises(ValueError):
        P.cells_of(100)


def test_prepare_rejects_a_null_handle():
    lib = _lib.load()
    seeds = np.zeros(1, dtype=np.int32)
    target = np.zeros(1)
    assert lib.ljmd_batch_prepare(None, seeds.ctypes.data_as(_lib.c_int32_p), target.ctypes.data_as(_lib.c_double_p), 0,
                                  None, None) == _lib.LJMD_ERR_INVALID_ARG
    assert "ljmd_batch_prepare" in _lib.batch_last_error()
    assert lib.ljmd_batch_prepare(None, None, None, -1, None, None) == _lib.LJMD_ERR_INVALID_ARG


def _unopened(n_replicas, n):
    """a BatchEngine whose handle was never created: the checks below run before any library call"""
    eng = object.__new__(BatchEngine)
    eng._lib = _lib.load()
    eng.params = md_types.init_params(n, synthetic.box_length(n), 0.005, 0.49 * synthetic.box_length(n))
    eng.n_replicas = n_replicas
    eng._h = None
    return eng


def test_batch_engine_prepare_checks_before_the_library():
    eng = _unopened(4, 108)
    for bad in (1.5, "7", None, True, [1.0, 2.0, 3.0, 4.0], np.array([True] * 4)):
        with pytest.raises(TypeError, match="seeds"):
            eng.prepare(bad, -500.0)
    for bad in ([1, 2, 3], np.zeros((4, 1), dtype=np.int64), np.zeros((2, 2), dtype=np.int32)):
        with pytest.raises(ValueError, match="seeds"):
            eng.prepare(bad, -500.0)
    for bad in (2 ** 31, -2 ** 31 - 1, [1, 2, 3, 2 ** 40]):
        with pytest.raises(ValueError, match="int32"):
            eng.prepare(bad, -500.0)
    for bad in ("x", None, True, [1j] * 4):
        with pytest.raises(TypeError, match="target_total_energy"):
            eng.prepare(1, bad)
    for bad in ([-500.0] * 3, np.zeros((4, 2))):
        with pytest.raises(ValueError, match="target_total_energy"):
            eng.prepare(1, bad)
    for bad in (1.0, "3", None, False):
        with pytest.raises(TypeError, match="warmup_steps"):
            eng.prepare(1, -500.0, warmup_steps=bad)
    with pytest.raises(ValueError, match="warmup_steps"):
        eng.prepare(1, -500.0, warmup_steps=2 ** 31)
    # what passes the checks reaches the library, which refuses the handle that was never created
    with pytest.raises(_lib.LjmdError) as ei:
        eng.prepare([1, 2, 3, 4], -500.0)
    assert ei.value.code == _lib.LJMD_ERR_INVALID_ARG and "ljmd_batch_prepare" in ei.value.message
    with pytest.raises(_lib.LjmdError):
        eng.prepare(np.int32(-7), np.full(4, -500.0), warmup_steps=np.int64(3))


def test_prepare_host_code_under_sanitizers():
    """guards, launches per kernel class, scale factors, warm-up without snapshots, no state after a target below the
    lattice energy, poison and recovery: tests/prepare_host/prepare_host.cpp checks itself"""
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc absent: the program cannot be built")
    here = ROOT / "tests" / "prepare_host"
    subprocess.run(["make", "-C", str(here)], check=True, capture_output=True, timeout=600)
    env = {k: v for k, v in os.environ.items() if not k.startswith("LJMD_")}
    env.update(FAKEHIP_DEVICES="1", ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:exitcode=23",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1:exitcode=24")
    out = subprocess.run([str(here / "prepare_host")], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-6000:])
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error:" not in out.stderr, out.stderr[-6000:]
    assert out.stdout.strip().splitlines()[-1] == "prepare_host: ok" and "FAILED" not in out.stdout
