"""CPU-only: the batch engine's C ABI (include/ljmd.h, ljmd_batch_*) rejects bad arguments before it probes for a
device, fails loudly without one, and the Python BatchEngine checks array shapes before it calls the library."""
import ctypes as C

import numpy as np
import pytest

import ljmd_amd
from ljmd_amd import BatchEngine, _lib, md_types, synthetic

L = 10.0


def _create(n_replicas=4, n=108, box_length=L, dt=0.005, rc=4.0, mode=0, device=0):
    h = C.c_void_p()
    rc_ = _lib.load().ljmd_batch_create(C.byref(h), n_replicas, n, box_length, dt, rc, mode, device)
    return rc_, h


@pytest.mark.parametrize("kw", [
    dict(n=0), dict(n=-5), dict(box_length=-1.0), dict(box_length=0.0), dict(rc=0.0), dict(rc=5.0), dict(rc=6.0),
    dict(dt=0.0), dict(dt=-0.1),                                          # the guards of ljmd_create
    dict(n_replicas=0), dict(n_replicas=-3),                              # no replicas
    dict(n=4097), dict(n=100000),                                         # n > LJMD_BATCH_MAX_N
    dict(mode=1), dict(mode=2), dict(mode=7),                             # fp64 only
    dict(rc=5.0 * (1.0 - 1e-10)), dict(rc=0.5 * L * (1.0 - 0.5e-9)),      # rc > (1 - 1e-9) L/2, still < L/2
])
def test_batch_create_guards_before_device_probe(kw):
    """the guards run first: LJMD_ERR_INVALID_ARG whether or not a device is present"""
    rc_, h = _create(**kw)
    assert rc_ == _lib.LJMD_ERR_INVALID_ARG, (kw, rc_)
    assert not h.value
    msg = _lib.batch_last_error()
    assert msg.startswith("ljmd_batch_create:"), msg


def test_batch_create_out_null():
    lib = _lib.load()
    assert lib.ljmd_batch_create(None, 4, 108, L, 0.005, 4.0, 0, 0) == _lib.LJMD_ERR_INVALID_ARG


def test_batch_limits_are_accepted_by_the_guards():
    """n = LJMD_BATCH_MAX_N and rc = (1 - 1e-9) L/2 pass the guards: without a device they reach the probe"""
    lib = _lib.load()
    if lib.ljmd_device_count() > 0:
        pytest.skip("a HIP device is present")
    for kw in (dict(n=4096), dict(rc=(1.0 - 1e-9) * 0.5 * L), dict(n_replicas=1), dict(n=1)):
        rc_, h = _create(**kw)
        assert rc_ == _lib.LJMD_ERR_NO_DEVICE, (kw, rc_)


def test_batch_no_device_fails_loudly():
    lib = _lib.load()
    if lib.ljmd_device_count() > 0:
        pytest.skip("a HIP device is present")
    rc_, h = _create()
    assert rc_ == _lib.LJMD_ERR_NO_DEVICE and not h.value
    assert "no HIP device" in _lib.batch_last_error() and "no CPU path" in _lib.batch_last_error()
    p = md_types.init_params(108, 5.129927840030091, 0.005, 0.49 * 5.129927840030091)
    with pytest.raises(ljmd_amd.LjmdError) as ei:
        BatchEngine(p, 8)
    assert ei.value.code == _lib.LJMD_ERR_NO_DEVICE and "no CPU path" in ei.value.message


def test_batch_entry_points_reject_a_null_handle():
    lib = _lib.load()
    assert lib.ljmd_batch_set_state(None, *[None] * 6) == _lib.LJMD_ERR_INVALID_ARG
    assert lib.ljmd_batch_set_accel(None, *[None] * 3) == _lib.LJMD_ERR_INVALID_ARG
    assert lib.ljmd_batch_set_unwrapped(None, *[None] * 3) == _lib.LJMD_ERR_INVALID_ARG
    assert lib.ljmd_batch_get_state(None, *[None] * 12) == _lib.LJMD_ERR_INVALID_ARG
    assert lib.ljmd_batch_compute_forces(None, None, None, None) == _lib.LJMD_ERR_INVALID_ARG
    assert lib.ljmd_batch_kinetic_energy(None, None) == _lib.LJMD_ERR_INVALID_ARG
    assert lib.ljmd_batch_steps(None, 10, 1, None, None, None, None) == _lib.LJMD_ERR_INVALID_ARG
    assert lib.ljmd_batch_set_tail_corrections(None, 0) == _lib.LJMD_ERR_INVALID_ARG
    assert lib.ljmd_batch_profile_read(None, None, None) == _lib.LJMD_ERR_INVALID_ARG
    lib.ljmd_batch_destroy(None)                                            # no-op


def _unopened(n_replicas, n):
    """a BatchEngine whose handle was never created: the shape checks run before any library call"""
    eng = object.__new__(BatchEngine)
    eng._lib = _lib.load()
    eng.params = md_types.init_params(n, synthetic.box_length(n), 0.005, 0.49 * synthetic.box_length(n))
    eng.n_replicas = n_replicas
    eng._h = None
    return eng


@pytest.mark.parametrize("shape", [(4, 107), (3, 108), (432,), (108, 4), (4, 108, 1)])
def test_batch_engine_rejects_wrongly_shaped_arrays(shape):
    eng = _unopened(4, 108)
    good = np.zeros((4, 108))
    bad = np.zeros(shape)
    with pytest.raises(ValueError, match=r"shape \(4, 108\)"):
        eng.set_state(good, good, bad, good, good, good)
    with pytest.raises(ValueError, match=r"shape \(4, 108\)"):
        eng.set_accel(bad, None, None)
    with pytest.raises(ValueError, match=r"shape \(4, 108\)"):
        eng.set_unwrapped(good, bad, good)


def test_batch_engine_rejects_a_sample_interval_that_does_not_divide():
    eng = _unopened(2, 108)
    with pytest.raises(ValueError, match="multiple of sample_every"):
        eng.steps(10, sample_every=3)
    with pytest.raises(ValueError, match="multiple of sample_every"):
        eng.steps(10, sample_every=0)


def test_batch_header_documents_the_contract():
    from conftest import ROOT
    text = (ROOT / "include" / "ljmd.h").read_text()
    assert "#define LJMD_BATCH_MAX_N 4096" in text
    for phrase in ("24 n bytes", "generic-kernel fallback", "ljmd_batch_steps", "bitwise"):
        assert phrase in text, phrase
