"""The inputs of tests/test_gpu_hostile.py, checked on the CPU so that a GPU failure cannot be blamed on them: sizes,
minimum separation, wrapping, raw spans, a well-conditioned energy, tile pairs that the mask can skip, finite forces,
and that one dropped pair would be seen at the bounds the GPU tests use."""
import numpy as np
import pytest

import hostile_configs as hc
from ljmd_amd import synthetic

S_CASES = {"droplet": lambda: hc.droplet(hc.DROPLET_S), "slab": lambda: hc.slab(hc.SLAB_S), "sheets": lambda: hc.sheets(hc.SHEETS_S)}
M_CASES = {"droplet": lambda: hc.droplet(hc.DROPLET_M), "slab": lambda: hc.slab(hc.SLAB_M)}
_cache = {}


def cfg(size, name):
    if (size, name) not in _cache:
        _cache[size, name] = (S_CASES if size == "S" else M_CASES)[name]()
    return _cache[size, name]


def oracle_forces(oracle, p, r):
    po = oracle.derive_params(p.n, p.box_length, p.dt, p.rc)
    e, d, dd, ax, ay, az = oracle.compute_forces(po, r[0].copy(), r[1].copy(), r[2].copy())
    return e, d, dd, np.stack([ax, ay, az])


ALL = [("S", "droplet"), ("S", "slab"), ("S", "sheets"), ("M", "droplet"), ("M", "slab")]


@pytest.mark.parametrize("size,name", ALL)
def test_size_wrapping_separation_and_conditioning(oracle, size, name):
    p, r, v = cfg(size, name)
    n, L = p.n, p.box_length
    assert r.shape == v.shape == (3, n) and r.dtype == v.dtype == np.float64
    if size == "S":
        assert 4200 <= n <= 6000, n
        if name != "sheets":
            assert n % 64 != 0, n
    else:
        assert 16500 <= n <= 20000 and n % 256 != 0, n
    assert p.rc == 0.49 * L
    assert r.min() >= 0.0 and r.max() < L
    assert np.abs(v.sum(axis=1)).max() < 1e-9 and abs(0.5 * np.sum(v * v) - 1.5 * n) < 1e-9 * n
    dmin, sum_abs = hc.pair_pass(r, L, p.rc)
    e, d, dd, a = oracle_forces(oracle, p, r)
    print(f"{name} {size}: n = {n}, L = {L}, min distance {dmin:.4f}, |epot| / sum|terms| = {abs(e) / sum_abs:.3f}, max|a| = {np.abs(a).max():.3g}")
    assert dmin >= 0.9, dmin
    assert abs(e) >= 0.5 * sum_abs, (e, sum_abs)
    assert np.all(np.isfinite(a)) and np.abs(a).max() < 1e4


def test_caller_order_is_shuffled():
    for name in S_CASES:
        p, r, v = cfg("S", name)
        # a lattice order would be monotonic along its slowest axis; a shuffle has about n / 2 descents
        assert np.count_nonzero(np.diff(r[0]) < 0) > p.n // 3


def test_sheets_has_exactly_two_z_values():
    p, r, v = cfg("S", "sheets")
    assert sorted(set(r[2].tolist())) == [0.0, p.box_length - 1.0]
    assert np.count_nonzero(r[2] == 0.0) == p.n // 2


@pytest.mark.parametrize("name", ["droplet", "slab"])
def test_mask_can_skip_tile_pairs(name):
    """64-particle tiles of a spatial sort: how many tile pairs have boxes further apart than the cutoff.  At rc = 0.49 L
    the minimum-image distance of two boxes cannot exceed sqrt(3) (L / 2 - width), and the dense part of either
    configuration lies within 0.6 L of itself, so only a few per cent of its tile pairs can be skipped; the 30 % condition
    is met at the short cutoff rc = 0.15 L that the GPU tests also run, and both fractions are printed."""
    p, r, v = cfg("S", name)
    f49, T = hc.tile_skip_fraction(r, p.box_length, 0.49 * p.box_length)
    f15, _ = hc.tile_skip_fraction(r, p.box_length, 0.15 * p.box_length)
    print(f"{name} S: {T} tiles, box gap > rc for {f49:.3f} of the tile pairs at rc = 0.49 L, {f15:.3f} at rc = 0.15 L")
    assert f15 >= 0.30


@pytest.mark.parametrize("size,name", [("S", "droplet"), ("S", "slab"), ("M", "slab")])
def test_raw_images_span_and_equal_forces(oracle, size, name):
    p, r, v = cfg(size, name)
    L = p.box_length
    pr, x, vr = hc.raw_images((p, r, v))
    assert pr is p and np.array_equal(vr, v)
    k = (x - r) / L
    assert np.abs(k - np.rint(k)).max() < 1e-12 and set(np.unique(np.rint(k)).tolist()) == {-1.0, 0.0, 1.0}
    assert x.min() > -0.69 * L and x.max() < 1.69 * L
    span = (x.max(axis=1) - x.min(axis=1)) / L
    print(f"raw_images({name} {size}): spans / L = {span}")
    assert np.all(span < 2.4)
    # the slab occupies |x| < 0.15 L only: whole-L moves inside (-0.69 L, 1.69 L) reach -0.15 L .. 1.15 L on that axis
    need = [1, 2] if name == "slab" else [0, 1, 2]
    assert np.all(span[need] > 2.3), span
    if name == "slab":
        assert 1.25 < span[0] < 1.31
    if size == "S":
        e, d, dd, a = oracle_forces(oracle, p, r)
        ex, dx, ddx, ax = oracle_forces(oracle, p, x)
        assert np.abs(ax - a).max() <= 1e-12 * np.abs(a).max()
        assert abs(ex - e) <= 1e-12 * abs(e) and abs(dx - d) <= 1e-12 * abs(d) and abs(ddx - dd) <= 1e-12 * abs(dd)


@pytest.mark.parametrize("n", [500, 1372])
def test_raw_images_of_the_uniform_small_systems(n):
    p, r, v = synthetic.make_config(n)
    _, x, _ = hc.raw_images((p, r, v))
    span = (x.max(axis=1) - x.min(axis=1)) / p.box_length
    # both are fcc lattices (5 and 7 cells): planes every L / 10 and L / 14, so whole-L moves inside (-0.69 L, 1.69 L)
    # reach -0.6 L .. 1.6 L and -0.643 L .. 1.643 L, not the 2.3 L of the large configurations
    assert np.all(span > 2.2) and np.all(span < 2.4), span


def test_one_dropped_pair_across_a_face_would_be_seen(oracle):
    """The GPU tests' bounds against what ONE wrongly skipped pair does: take the droplet at S, find the in-cutoff pairs
    whose minimum image goes through a face, and remove the WEAKEST of them (the one nearest the cutoff) from the sums.
    The fp64 bounds (1e-12 relative on the scalars, 1e-12 max|a| on the accelerations) must see it, and the fixed-point
    sums of the reproducible mode, g(r) and the stress words change by whole quanta (2^-64) for any pair inside rc."""
    p, r, v = cfg("S", "droplet")
    L, rc = p.box_length, p.rc
    e, d, dd, a = oracle_forces(oracle, p, r)
    rt = r.T
    best = None
    for i0 in range(0, p.n, 512):
        dv = rt[i0:i0 + 512, None, :] - rt[None, :, :]
        img = np.rint(dv / L)
        dv -= L * img
        r2 = np.einsum("ijk,ijk->ij", dv, dv)
        ok = (r2 < rc * rc) & np.any(img != 0.0, axis=2)
        if ok.any():
            r2m = np.where(ok, r2, 0.0)
            i, j = np.unravel_index(np.argmax(r2m), r2m.shape)
            if best is None or r2m[i, j] > best[0]:
                best = (r2m[i, j], i0 + i, j, dv[i, j].copy())
    r2, i, j, dv = best
    u3 = r2 ** -3
    u6 = u3 * u3
    de, dd1, ddd = 4.0 * (u6 - u3), 24.0 * (u3 - 2.0 * u6), 24.0 * (26.0 * u6 - 7.0 * u3)
    da = 24.0 * (2.0 * u6 - u3) / r2 * np.abs(dv).max()
    print(f"weakest cross-face pair ({i}, {j}) at r = {np.sqrt(r2):.4f} of rc = {rc:.4f}: d epot / epot = {abs(de / e):.2e}, "
          f"d d_epot / d_epot = {abs(dd1 / d):.2e}, d dd_epot / dd_epot = {abs(ddd / dd):.2e}, d a / max|a| = {abs(da) / np.abs(a).max():.2e}")
    assert abs(de) > 1e-12 * abs(e) and abs(dd1) > 1e-12 * abs(d) and abs(ddd) > 1e-12 * abs(dd)
    assert abs(da) > 1e-12 * np.abs(a).max()
    # integer sums: the smallest term of any pair inside rc is u^6 > rc^-12, many quanta of 2^-64; a pair counts 2 in g(r)
    for name in S_CASES:
        assert np.rint(cfg("S", name)[0].rc ** -12 * 2.0 ** 64) >= 64.0
