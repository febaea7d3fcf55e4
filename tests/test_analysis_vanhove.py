"""CPU-only: the numpy helpers that turn the van Hove counts of Engine.vanhove_read into G_s(r, tau), F_s(k, tau) and
alpha_2(tau) (ljmd_amd.analysis)."""
import math

import numpy as np
import pytest

from ljmd_amd import analysis


def _histogram(disp, nbins, dr):
    """disp [rows, n] displacement lengths -> hist [rows, nbins + 1], the overflow column last"""
    hist = np.zeros((disp.shape[0], nbins + 1), dtype=np.uint64)
    for l, d in enumerate(disp):
        b = np.minimum(np.floor(d / dr).astype(np.int64), nbins)
        hist[l] = np.bincount(b, minlength=nbins + 1)
    return hist


def test_van_hove_self_integrates_to_one_minus_overflow():
    rng = np.random.Generator(np.random.PCG64(5))
    n, nbins, dr = 700, 50, 0.02
    disp = np.abs(rng.normal(0.0, [[0.1], [0.4], [0.9], [1.0]], size=(4, n)))
    counts = np.array([3, 2, 1, 0])
    hist = _histogram(disp, nbins, dr) * counts[:, None].astype(np.uint64)
    centres, g, overflow = analysis.van_hove_self(hist, counts, n, dr)
    b = np.arange(nbins, dtype=np.float64)
    shell = 4.0 * math.pi / 3.0 * ((b + 1.0) ** 3 - b ** 3) * dr ** 3
    assert g.shape == (4, nbins) and overflow.shape == (4,) and np.array_equal(centres, (b + 0.5) * dr)
    integral = (g * shell).sum(axis=1)
    assert np.all(np.abs(integral[:3] - (1.0 - overflow[:3])) <= 64 * np.finfo(float).eps)     # nbins roundings
    assert overflow[0] == 0.0 and 0.0 < overflow[1] < overflow[2] < 1.0
    assert np.array_equal(overflow[:3], hist[:3, -1] / (n * counts[:3]))
    assert not g[3].any() and overflow[3] == 0.0                                             # a lag nobody met
    assert g[0].argmax() < g[1].argmax() or g[0].max() > g[1].max()
    with pytest.raises(ValueError):
        analysis.van_hove_self(hist, counts[:3], n, dr)


def test_non_gaussian_parameter_is_the_formula_bitwise():
    rng = np.random.Generator(np.random.PCG64(6))
    r2 = rng.random(40) * 3.0
    r4 = r2 * r2 * (5.0 / 3.0) * (1.0 + 0.3 * rng.random(40))
    r2[0] = r4[0] = 0.0                                                                      # lag 0
    got = analysis.non_gaussian_parameter(r2, r4)
    want = [0.0] + [3.0 * float(b) / (5.0 * (float(a) * float(a))) - 1.0 for a, b in zip(r2[1:], r4[1:])]
    assert got.tobytes() == np.array(want).tobytes()
    assert abs(analysis.non_gaussian_parameter(np.array([3.0]), np.array([15.0]))[0]) == 0.0   # Gaussian: <r^4> = 5/3 <r^2>^2


def test_self_intermediate_scattering_against_the_direct_mean():
    """|d/dx (sin x / x)| < 1/2 and a bin centre lies within dr / 2 of the displacement: every term, hence the mean, is
    within k dr / 4 of sinc(k |d|)"""
    rng = np.random.Generator(np.random.PCG64(7))
    n, nbins, dr = 900, 200, 0.01
    d = rng.normal(0.0, [[0.05], [0.2], [0.35]], size=(3, 3, n))
    length = np.sqrt((d * d).sum(axis=1))                                                    # [3 lags, n]
    assert length.max() < nbins * dr                                                         # nothing overflows
    counts = np.array([1, 1, 1])
    hist = _histogram(length, nbins, dr)
    ks = np.array([0.5, 2.0, 7.0, 20.0])
    f, overflow = analysis.self_intermediate_scattering(hist, counts, n, dr, ks)
    assert f.shape == (4, 3) and not overflow.any()
    for a, k in enumerate(ks):
        direct = np.sinc(k * length / math.pi).mean(axis=1)
        assert np.all(np.abs(f[a] - direct) <= k * dr / 4.0), (k, f[a], direct)
        one, _ = analysis.self_intermediate_scattering(hist, counts, n, dr, float(k))
        assert one.shape == (3,) and one.tobytes() == f[a].tobytes()
    assert np.all(f[0] > f[3])                                                               # decays with k
    zero, _ = analysis.self_intermediate_scattering(hist, counts, n, dr, 0.0)
    assert np.allclose(zero, 1.0, rtol=0, atol=1e-12)
