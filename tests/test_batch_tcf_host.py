"""CPU-only: the MSD / VACF accumulation of the batch engine (include/ljmd.h, ljmd_batch_tcf_*).  The definition's CPU
model (tests/tcf_model.py) against the reference's own analysis output, the entry points' NULL-handle guards,
ljmd_tcf_from_exact against R(S) / (n count) bit for bit, and the checks BatchEngine makes before it calls the library."""
import ctypes as C

import numpy as np
import pytest

import tcf_model
from conftest import GOLDEN
from ljmd_amd import BatchEngine, _lib, analysis, io_formats, md_types, synthetic
from reproducible_model import R

PAIRS = [(8, 1), (4, 2), (5, 3), (7, 2), (3, 5), (1, 1), (6, 6)]       # (max_lag, origin_stride)


@pytest.fixture(scope="module")
def ref_run():
    _, snaps = io_formats.read_rva(GOLDEN / "ref_run_n108_oi100" / "rva.dat")
    return snaps[:, 1], snaps[:, 2]                                    # ru, v: [9, 3, 108]


def _model(ru, v, max_lag, stride):
    m = tcf_model.TcfModel(max_lag, stride)
    for s in range(ru.shape[0]):
        m.push(ru[s], v[s])
    assert not m.range_flag
    return m


def _close(a, b):
    return a.shape == b.shape and np.max(np.abs(a - b)) <= 1e-13 * np.max(np.abs(b))


@pytest.mark.parametrize("max_lag, stride", PAIRS)
def test_model_equals_the_reference_arithmetic(ref_run, golden, max_lag, stride):
    ru, v = ref_run
    n_snap, n = ru.shape[0], ru.shape[2]
    assert (n_snap, n) == (9, 108)
    m = _model(ru, v, max_lag, stride)
    assert np.array_equal(m.counts, tcf_model.reference_counts(n_snap, max_lag, stride))
    assert m.counts[0] >= 1
    msd, vacf = m.result(tcf_model.MSD, n), m.result(tcf_model.VACF, n)
    assert _close(msd, analysis.compute_msd_tau_timeorig(ru[:, 0], ru[:, 1], ru[:, 2], max_lag, stride))
    assert _close(vacf, analysis.compute_vacf_tau_timeorig(v[:, 0], v[:, 1], v[:, 2], max_lag, stride))
    g = golden("analysis_n108")
    if (max_lag, stride) == (8, 1):                                    # the reference module's own output
        assert _close(msd, g["msd"]) and _close(vacf, g["vacf"])
    if (max_lag, stride) == (4, 2):
        assert _close(msd, g["msd_lag4_stride2"])


def test_model_keeps_sums_over_trajectories_and_drops_origins(ref_run):
    ru, v = ref_run
    once = _model(ru, v, 4, 2)
    twice = _model(ru, v, 4, 2)
    twice.new_trajectory()
    twice.push(ru[0], v[0])                                            # no origin is live: contributes nothing
    assert twice.S == once.S and np.array_equal(twice.counts, once.counts)
    for s in range(1, ru.shape[0]):
        twice.push(ru[s], v[s])
    assert twice.S == [[2 * x for x in row] for row in once.S] and np.array_equal(twice.counts, 2 * once.counts)


def test_tcf_entry_points_reject_a_null_handle():
    lib = _lib.load()
    assert lib.ljmd_batch_tcf_configure(None, 10, 1, 0) == _lib.LJMD_ERR_INVALID_ARG
    assert "ljmd_batch_tcf_configure" in _lib.batch_last_error()
    assert lib.ljmd_batch_tcf_accumulate(None) == _lib.LJMD_ERR_INVALID_ARG
    assert "ljmd_batch_tcf_accumulate" in _lib.batch_last_error()
    assert lib.ljmd_batch_tcf_read(None, None, None, None, None) == _lib.LJMD_ERR_INVALID_ARG
    assert "ljmd_batch_tcf_read" in _lib.batch_last_error()
    assert lib.ljmd_batch_tcf_read_exact(None, None, None, None) == _lib.LJMD_ERR_INVALID_ARG
    assert "ljmd_batch_tcf_read_exact" in _lib.batch_last_error()
    assert lib.ljmd_batch_tcf_reset(None) == _lib.LJMD_ERR_INVALID_ARG
    assert "ljmd_batch_tcf_reset" in _lib.batch_last_error()


def _from_exact(S: int, n: int, count: int) -> float:
    words = np.array([(S >> (64 * k)) & (2 ** 64 - 1) for k in range(3)], dtype=np.uint64).view(np.int64)
    out = C.c_double(np.nan)
    assert _lib.load().ljmd_tcf_from_exact(words.ctypes.data_as(_lib.c_int64_p), n, count, C.byref(out)) == _lib.LJMD_OK
    return out.value


def test_from_exact_is_one_rounding_and_one_division():
    tie_even = (2 ** 53 + 1) << 20            # 54 significant bits, the last one set: a tie, rounds to even (down)
    tie_odd = (2 ** 53 + 3) << 20             # ... rounds to even (up)
    cases = [0, 1, -1, 12345678901234567890123, -98765432109876543210987, 3 << 130, -(5 << 131) + 7, (1 << 150) - 1,
             tie_even, -tie_even, tie_odd, tie_even + 1, tie_even - 1, (2 ** 53 + 1) << 100, 2 ** 191 - 1, -2 ** 191]
    assert R(tie_even) == float(2 ** 53 << 20) / 2.0 ** 64 and R(tie_odd) == float((2 ** 53 + 4) << 20) / 2.0 ** 64
    for S in cases:
        for n, count in ((108, 7), (1, 1), (4096, 1000003)):
            got, want = _from_exact(S, n, count), R(S) / (n * count)
            assert np.float64(got).tobytes() == np.float64(want).tobytes(), (S, n, count, got, want)
        assert _from_exact(S, 108, 0) == 0.0 and not np.signbit(_from_exact(S, 108, 0))
    lib = _lib.load()
    out = C.c_double()
    assert lib.ljmd_tcf_from_exact(None, 1, 1, C.byref(out)) == _lib.LJMD_ERR_INVALID_ARG
    assert "ljmd_tcf_from_exact" in _lib.batch_last_error()


def _unopened(n_replicas, n):
    """a BatchEngine whose handle was never created: the checks below run before any library call"""
    eng = object.__new__(BatchEngine)
    eng._lib = _lib.load()
    eng.params = md_types.init_params(n, synthetic.box_length(n), 0.005, 0.49 * synthetic.box_length(n))
    eng.n_replicas = n_replicas
    eng._h = None
    return eng


def test_batch_engine_tcf_checks_before_the_library():
    eng = _unopened(4, 108)
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
