"""CPU-only: batch handles whose replicas each have their own (n, L, dt, rc) (ljmd_batch_create_per_replica,
include/ljmd.h).  Every replica's guards run before the device probe and name the replica; the Python
PerReplicaBatchEngine checks list lengths and (n_b,) shapes before any library call; the host launch planning
(groups by kernel class, chunks, steps per launch, group streams) runs under AddressSanitizer + UBSan against the fake
HIP runtime of tests/fakehip; and bin/md_simulation_many_gpu stops on a bad per-run parameters file before it touches
the device."""
import ctypes as C
import glob
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from ljmd_amd import BatchEngine, PerReplicaBatchEngine, _lib, synthetic

PKG = ROOT / "molecular-dynamics-simulation---lennard-jones-monoatomic-fluid_amd"
ASAN_LIB = PKG / "csrc" / "obj" / "libljmd_asan.so"
FAKE = ROOT / "tests" / "fakehip" / "libfakehip.so"

GOOD = dict(n=[108, 500, 4000], box_length=[5.0, 8.0, 16.0], dt=[0.005, 0.002, 0.001], rc=[2.4, 3.9, 7.8])


def _create(n_replicas=None, mode=0, device=0, null=None, **over):
    f = {k: list(v) for k, v in GOOD.items()}
    for k, (b, x) in over.items():
        f[k][b] = x
    B = len(f["n"]) if n_replicas is None else n_replicas
    arrs = {"n": (C.c_int32 * 3)(*f["n"])}
    for k in ("box_length", "dt", "rc"):
        arrs[k] = (C.c_double * 3)(*f[k])
    if null:
        arrs[null] = None
    h = C.c_void_p()
    rc_ = _lib.load().ljmd_batch_create_per_replica(C.byref(h), B, arrs["n"], arrs["box_length"], arrs["dt"],
                                                     arrs["rc"], mode, device)
    return rc_, h


@pytest.mark.parametrize("b", [0, 1, 2])
@pytest.mark.parametrize("field,value", [
    ("n", 0), ("n", -3), ("n", 4097),
    ("box_length", 0.0), ("box_length", -1.0),
    ("dt", 0.0), ("dt", -0.001),
    ("rc", 0.0),
    ("rc", "just_above"),                  # rc just above (1 - 1e-9) L/2, still < L/2
    ("rc", "half"),                        # rc = L/2
])
def test_per_replica_guards_name_the_replica(b, field, value):
    if value == "just_above":
        value = 0.5 * GOOD["box_length"][b] * (1.0 - 0.5e-9)
    elif value == "half":
        value = 0.5 * GOOD["box_length"][b]
    rc_, h = _create(**{field: (b, value)})
    assert rc_ == _lib.LJMD_ERR_INVALID_ARG and not h.value, (field, value, rc_)
    msg = _lib.batch_last_error()
    assert msg.startswith(f"ljmd_batch_create_per_replica: replica {b}:"), msg


@pytest.mark.parametrize("kw", [dict(mode=1), dict(mode=2), dict(mode=7), dict(n_replicas=0), dict(n_replicas=-2),
                                dict(null="n"), dict(null="box_length"), dict(null="dt"), dict(null="rc")])
def test_per_replica_guards_before_device_probe(kw):
    rc_, h = _create(**kw)
    assert rc_ == _lib.LJMD_ERR_INVALID_ARG and not h.value, (kw, rc_)
    assert _lib.batch_last_error().startswith("ljmd_batch_create_per_replica:")


def test_per_replica_out_null():
    n = (C.c_int32 * 1)(108)
    d = (C.c_double * 1)(5.0)
    assert _lib.load().ljmd_batch_create_per_replica(None, 1, n, d, d, d, 0, 0) == _lib.LJMD_ERR_INVALID_ARG


def test_per_replica_limits_reach_the_device_probe():
    lib = _lib.load()
    if lib.ljmd_device_count() > 0:
        pytest.skip("a HIP device is present")
    for kw in (dict(), dict(n=(0, 4096)), dict(n=(1, 1)), dict(rc=(2, (1.0 - 1e-9) * 0.5 * 16.0)), dict(n_replicas=1)):
        rc_, h = _create(**kw)
        assert rc_ == _lib.LJMD_ERR_NO_DEVICE and not h.value, (kw, rc_)
        assert _lib.batch_last_error().startswith("ljmd_batch_create_per_replica: no HIP device")
    with pytest.raises(_lib.LjmdError) as ei:
        BatchEngine.per_replica([synthetic.make_config(n)[0] for n in (108, 256)])
    assert ei.value.code == _lib.LJMD_ERR_NO_DEVICE


def test_offsets_rejects_null():
    assert _lib.load().ljmd_batch_offsets(None, None) == _lib.LJMD_ERR_INVALID_ARG


def _unopened(ns):
    """a PerReplicaBatchEngine whose handle was never created: the shape checks run before any library call"""
    eng = object.__new__(PerReplicaBatchEngine)
    eng._lib = _lib.load()
    eng.params_list = [synthetic.make_config(n)[0] for n in ns]
    eng.n_replicas = len(ns)
    eng.offsets = np.concatenate([[0], np.cumsum(ns)]).astype(np.int64)
    eng._h = None
    return eng


def test_per_replica_engine_rejects_wrong_lists_and_shapes():
    eng = _unopened([32, 108, 500])
    good = [np.zeros(32), np.zeros(108), np.zeros(500)]
    for bad, match in (([np.zeros(32), np.zeros(108)], "list of 3 arrays"),
                       (good + [np.zeros(4)], "list of 3 arrays"),
                       (np.zeros((3, 108)), "list of 3 arrays"),
                       ([np.zeros(32), np.zeros(107), np.zeros(500)], r"replica 1 must have shape \(108,\)"),
                       ([np.zeros(32), np.zeros(108), np.zeros((500, 1))], r"replica 2 must have shape \(500,\)"),
                       ([np.zeros(108), np.zeros(108), np.zeros(500)], r"replica 0 must have shape \(32,\)")):
        with pytest.raises(ValueError, match=match):
            eng.set_state(good, good, bad, good, good, good)
        with pytest.raises(ValueError, match=match):
            eng.set_accel(bad, None, None)
        with pytest.raises(ValueError, match=match):
            eng.set_unwrapped(good, good, bad)


SCRIPT = r"""
import ctypes as C, os, sys
sys.path.insert(0, %(root)r)
import numpy as np
from ljmd_amd import BatchEngine, synthetic
fake = C.CDLL(%(fake)r)
fake.fakehip_kernel_launches.restype = C.c_long
ns = [32, 4000, 108, 500, 1372, 864, 200, 2048, 2916, 64]
cfg = [synthetic.make_config(n, seed=40 + i) for i, n in enumerate(ns)]
for streams in ("1", "0"):
    os.environ["LJMD_BATCH_GROUP_STREAMS"] = streams
    with BatchEngine.per_replica([c[0] for c in cfg]) as eng:
        assert list(eng.offsets) == list(np.concatenate([[0], np.cumsum(ns)])), eng.offsets
        r = [[c[1][ax] for c in cfg] for ax in range(3)]
        v = [[c[2][ax] for c in cfg] for ax in range(3)]
        eng.set_state(*r, *v)
        st = eng.get_state()
        for ax in range(3):
            for b, n in enumerate(ns):
                assert st["r"][ax][b].shape == (n,) and np.array_equal(st["r"][ax][b], r[ax][b])
                assert np.array_equal(st["ru"][ax][b], r[ax][b]) and np.array_equal(st["v"][ax][b], v[ax][b])
                assert not st["a"][ax][b].any()
        e, d, dd = eng.compute_forces()
        assert e.shape == (len(ns),)
        assert eng.kinetic_energy().shape == (len(ns),)
        for nsteps, every, obs in ((40, 10, True), (30, 1, False), (7, 7, True)):
            l0 = fake.fakehip_kernel_launches()
            out = eng.steps(nsteps, every, observables=obs)
            prof = eng.profile_read()
            launched = fake.fakehip_kernel_launches() - l0
            assert launched == prof["launches"], (nsteps, launched, prof)
            assert launched > 5, launched               # five kernel classes, the n = 4000 group split into launches
            if obs:
                assert all(o.shape == (nsteps // every, len(ns)) for o in out)
        st = eng.get_state(("a", "v"))
        eng.set_accel(*st["a"])
        eng.set_unwrapped(*[[x + 1.0 for x in r[ax]] for ax in range(3)])
        assert np.array_equal(eng.get_state(("ru",))["ru"][1][3], r[1][3] + 1.0)
        eng.set_tail_corrections(False)
        eng.steps(4, 2)
print("per-replica host planning under sanitizers: ok")
"""


def test_per_replica_host_planning_under_sanitizers_with_fake_runtime():
    rt = sorted(glob.glob("/opt/rocm/lib/llvm/lib/clang/*/lib/linux/libclang_rt.asan-x86_64.so"))
    if not ASAN_LIB.exists() or not rt:
        pytest.skip("sanitizer build absent: make -C .../csrc asan")
    if not FAKE.exists():
        subprocess.run(["make", "-C", str(FAKE.parent)], check=True, capture_output=True)
    env = dict(os.environ, LD_PRELOAD=f"{rt[-1]} {FAKE}", LJMD_LIBRARY=str(ASAN_LIB), FAKEHIP_DEVICES="1",
               ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:exitcode=23",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1:exitcode=24")
    for k in [k for k in env if k.startswith("LJMD_") and k != "LJMD_LIBRARY"]:
        del env[k]
    out = subprocess.run([sys.executable, "-c", SCRIPT % {"root": str(ROOT), "fake": str(FAKE)}], env=env,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-6000:])
    assert "per-replica host planning under sanitizers: ok" in out.stdout
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error:" not in out.stderr


def _params_text(k, total_steps, output_interval, warmup, dt, box, rc_over_L):
    return (f"k   total_steps   output_interval   warmup_steps\n{k}   {total_steps}   {output_interval}   {warmup}\n\n"
            f"dt        L     rc_over_L\n{dt!r}   {box!r}   {rc_over_L!r}\n\ntarget_total_energy\n-500.d0\n")


@pytest.mark.parametrize("case", ["steps_block", "too_large"])
def test_many_driver_stops_on_a_bad_per_run_parameters_file(tmp_path, case):
    exe = PKG / "bin" / "md_simulation_many_gpu"
    if not exe.exists():
        pytest.skip("Fortran driver not built")
    src = GOLDEN / "ref_run_n108_oi10"
    (tmp_path / "inputs").mkdir()
    shutil.copy(src / "input_simulation_parameters.txt", tmp_path / "inputs")
    (tmp_path / "outputs").mkdir()
    shutil.copy(src / "rv_init.dat", tmp_path / "outputs" / "rv_init.dat")
    run2 = tmp_path / "outputs" / "run_0002"
    run2.mkdir()
    if case == "steps_block":
        text = _params_text(3, 1000, 20, 100, 0.004, 5.2, 0.45)          # output_interval 20 instead of 10
        expect = "run_0002/input_simulation_parameters.txt: total_steps, output_interval and warmup_steps must equal"
    else:
        text = _params_text(11, 1000, 10, 100, 0.005, 18.0, 0.45)        # N = 4 * 11^3 = 5324
        expect = "run_0002/input_simulation_parameters.txt: N = 5324 exceeds LJMD_BATCH_MAX_N (4096)"
    (run2 / "input_simulation_parameters.txt").write_text(text)
    # no device: the driver must stop on the file before it touches one (HIP_VISIBLE_DEVICES hides any card)
    out = subprocess.run([str(exe)], cwd=tmp_path, capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, LJMD_RUNS="3", HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1"))
    text_out = out.stdout + out.stderr
    assert expect in text_out, text_out[-2000:]
    assert "ljmd:" not in text_out and "rva.dat" not in {p.name for p in run2.iterdir()}, text_out[-2000:]
