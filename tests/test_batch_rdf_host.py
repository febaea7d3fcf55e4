"""CPU-only: the g(r) entry points of the batch engine (include/ljmd.h, ljmd_batch_rdf_*) reject a NULL handle, the
Python BatchEngine checks what it can before it calls the library, and analysis.rdf_from_histogram is the
normalisation of analysis.compute_rdf, bit for bit."""
import numpy as np
import pytest

from ljmd_amd import BatchEngine, _lib, analysis, md_types, synthetic


def test_rdf_entry_points_reject_a_null_handle():
    lib = _lib.load()
    assert lib.ljmd_batch_rdf_configure(None, 200, None, 0) == _lib.LJMD_ERR_INVALID_ARG
    assert "ljmd_batch_rdf_configure" in _lib.batch_last_error()
    assert lib.ljmd_batch_rdf_accumulate(None) == _lib.LJMD_ERR_INVALID_ARG
    assert lib.ljmd_batch_rdf_read(None, None, None) == _lib.LJMD_ERR_INVALID_ARG
    assert lib.ljmd_batch_rdf_reset(None) == _lib.LJMD_ERR_INVALID_ARG
    assert "ljmd_batch_rdf_reset" in _lib.batch_last_error()


def _unopened(n_replicas, n):
    """a BatchEngine whose handle was never created: the checks below run before any library call"""
    eng = object.__new__(BatchEngine)
    eng._lib = _lib.load()
    eng.params = md_types.init_params(n, synthetic.box_length(n), 0.005, 0.49 * synthetic.box_length(n))
    eng.n_replicas = n_replicas
    eng._h = None
    return eng


def test_batch_engine_rdf_checks_before_the_library():
    eng = _unopened(4, 108)
    with pytest.raises(ValueError, match="rdf_configure"):
        eng.rdf_read()                                       # no bin count known yet: no shape to return
    for bad in (np.ones(3), np.ones(5), np.ones((4, 2)), np.ones((2, 4))):
        with pytest.raises(ValueError):
            eng.rdf_configure(200, rmax=bad)                 # neither a scalar nor one value per replica
    with pytest.raises(ValueError, match="rdf_configure"):
        eng.rdf_read()                                       # a refused configure leaves nothing behind


def test_rdf_from_histogram_is_compute_rdfs_normalisation(oracle):
    n, n_snap, nbins = 64, 5, 40
    p, _, _ = synthetic.make_config(n)
    L = p.box_length
    rng = np.random.Generator(np.random.PCG64(7))
    r = rng.random((3, n_snap, n)) * L
    for rmax in (0.5 * L, 0.3 * L):
        counts = np.zeros(nbins, dtype=np.uint64)
        for s in range(n_snap):
            oracle.rdf_histogram_np(r[0, s], r[1, s], r[2, s], L, nbins, rmax, counts)
        assert counts.sum() > 0
        centers, g = analysis.rdf_from_histogram(counts, n, L, nbins, rmax, n_snap)
        c_ref, g_ref = analysis.compute_rdf(r[0], r[1], r[2], L, nbins=nbins, rmax=rmax, subsample=False,
                                            histogram=oracle.rdf_histogram_np)
        assert np.array_equal(centers, c_ref) and np.array_equal(g, g_ref)
        assert g.dtype == np.float64 and g.shape == (nbins,) and g.max() > 0.0
