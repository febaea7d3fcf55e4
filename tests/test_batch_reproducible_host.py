"""CPU-only: the entry point that selects a batch handle's precision mode (ljmd_batch_set_precision, include/ljmd.h) and
its Python side.  The creators keep refusing every mode but LJMD_PRECISION_FP64; the reproducible mode is selected on
the handle, and BatchEngine refuses a mode no batch has before it calls the library."""
import ctypes as C

import numpy as np
import pytest

from ljmd_amd import BatchEngine, _lib, md_types, synthetic
from conftest import ROOT


def test_set_precision_rejects_a_null_handle():
    lib = _lib.load()
    assert lib.ljmd_batch_set_precision(None, _lib.PRECISION_FP64_REPRODUCIBLE) == _lib.LJMD_ERR_INVALID_ARG
    assert "NULL handle" in _lib.batch_last_error(None)
    assert lib.ljmd_batch_set_precision(None, _lib.PRECISION_FP64) == _lib.LJMD_ERR_INVALID_ARG


@pytest.mark.parametrize("mode", [1, 7])
def test_batch_engine_rejects_modes_no_batch_has_before_any_library_call(mode, monkeypatch):
    def no_library():
        raise AssertionError("the library was called")
    monkeypatch.setattr(_lib, "load", no_library)
    p = md_types.init_params(108, 10.0, 0.005, 4.0)
    with pytest.raises(ValueError, match="precision_mode"):
        BatchEngine(p, 4, precision_mode=mode)
    with pytest.raises(ValueError, match="precision_mode"):
        BatchEngine.per_replica([p, p], precision_mode=mode)


def test_header_names_the_call_and_the_batch_form_of_the_contract():
    text = (ROOT / "include" / "ljmd.h").read_text()
    assert "int ljmd_batch_set_precision(ljmd_batch_t *h, int32_t precision_mode);" in text
    for phrase in ("Reproducible batches", "exactly the\n * definition of LJMD_PRECISION_FP64_REPRODUCIBLE",
                   "LJMD_ERR_RANGE", "the creators take LJMD_PRECISION_FP64 only"):
        assert phrase in text, phrase
    assert "ljmd_batch_set_precision" in _lib.PROTOTYPES


def test_creators_still_refuse_the_reproducible_mode():
    lib = _lib.load()
    h = C.c_void_p()
    rc = lib.ljmd_batch_create(C.byref(h), 4, 108, 10.0, 0.005, 4.0, _lib.PRECISION_FP64_REPRODUCIBLE, 0)
    assert rc == _lib.LJMD_ERR_INVALID_ARG and not h.value
    assert "LJMD_PRECISION_FP64 only" in _lib.batch_last_error(None)
    n = np.array([108, 500], dtype=np.int32)
    box, dt, rcut = np.array([10.0, 12.0]), np.array([0.005, 0.004]), np.array([4.0, 3.0])
    dp = _lib.c_double_p
    rc = lib.ljmd_batch_create_per_replica(C.byref(h), 2, n.ctypes.data_as(_lib.c_int32_p), box.ctypes.data_as(dp),
                                           dt.ctypes.data_as(dp), rcut.ctypes.data_as(dp),
                                           _lib.PRECISION_FP64_REPRODUCIBLE, 0)
    assert rc == _lib.LJMD_ERR_INVALID_ARG and not h.value
    assert "LJMD_PRECISION_FP64 only" in _lib.batch_last_error(None)


def test_a_reproducible_batch_engine_opens_or_fails_loudly():
    """no CPU fall-back: without a device the creator's error comes through, whatever the mode asked for"""
    p, _, _ = synthetic.make_config(108)
    if _lib.load().ljmd_device_count() > 0:
        with BatchEngine(p, 2, precision_mode=_lib.PRECISION_FP64_REPRODUCIBLE) as eng:
            assert eng.precision_mode == _lib.PRECISION_FP64_REPRODUCIBLE
        return
    with pytest.raises(_lib.LjmdError) as ei:
        BatchEngine(p, 2, precision_mode=_lib.PRECISION_FP64_REPRODUCIBLE)
    assert ei.value.code == _lib.LJMD_ERR_NO_DEVICE
