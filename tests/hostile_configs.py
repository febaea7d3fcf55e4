"""Inhomogeneous and raw-coordinate start configurations for the pair kernels (pure numpy, seeded PCG64).

synthetic.make_config fills the box uniformly: equal tiles, no vacuum, no degenerate tile box, wrapped input.  The
generators here give what it cannot: a droplet in vapour wrapped through three faces, a slab in vacuum across a face,
two monolayers with exactly two z values, and wrapped configurations re-expressed in raw periodic images spanning
just under 2.4 L.  Every generator is built from jittered lattices, so the minimum separation holds by construction
(no rejection loop), shuffles the particles into a random caller order, and returns (SimParams, r[3, n], v[3, n])
with velocities as in make_config (uniform, centre of mass removed, T = 1).  The size argument is the box length L.
tests/test_hostile_configs.py proves the properties the GPU tests rely on.
"""
from __future__ import annotations

import numpy as np

from ljmd_amd import init_params

DT = 0.005
RC_OVER_L = 0.49

# box lengths of the two sizes the GPU tests use (n is asserted in tests/test_hostile_configs.py)
#   S: 4200 <= n <= 6000 -- the default Newton-3 kernel, one tile per row group
#   M: 16500 <= n <= 20000 -- two-tile row groups, the two-launch step, large enough for the mixed mode
DROPLET_S, DROPLET_M = 33.0, 52.0
SLAB_S, SLAB_M = 26.5, 39.7
SHEETS_S = 55.0


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _velocities(rng, n, temperature=1.0):
    v = rng.random((3, n)) - 0.5
    v -= v.mean(axis=1, keepdims=True)
    v *= np.sqrt(1.5 * n * temperature / (0.5 * np.sum(v * v)))
    return v


def _wrap(r, L):
    r = r - L * np.floor(r / L)
    r[r >= L] = 0.0
    return r


def _finish(rng, L, r, rc_over_L):
    """wrap, shuffle into caller order, draw velocities"""
    n = r.shape[1]
    r = _wrap(r, L)[:, rng.permutation(n)]
    return init_params(n, L, DT, rc_over_L * L), np.ascontiguousarray(r), np.ascontiguousarray(_velocities(rng, n))


def droplet(L=DROPLET_S, seed=101, rc_over_L=RC_OVER_L, radius_over_L=0.3):
    """A liquid droplet (simple cubic, rho = 0.9, +-5 % jitter) of radius 0.3 L centred on the box corner (0, 0, 0), so
    that it wraps through three faces, in a vapour (lattice at rho ~ 0.035, +-25 % jitter) that keeps 1 sigma away."""
    rng = _rng(seed)
    R = radius_over_L * L
    a = 0.9 ** (-1.0 / 3.0)
    k = int(np.ceil(R / a))
    g = np.arange(-k, k + 1, dtype=np.float64) * a
    site = np.stack(np.meshgrid(g, g, g, indexing="ij")).reshape(3, -1)
    site = site[:, np.sum(site * site, axis=0) <= R * R]
    dense = site + (rng.random(site.shape) - 0.5) * (2.0 * 0.05 * a)       # at most 0.05 sqrt(3) a = 0.09 past R
    m = int(round(L / 0.035 ** (-1.0 / 3.0)))
    av = L / m
    g = (np.arange(m, dtype=np.float64) + 0.5) * av
    site = np.stack(np.meshgrid(g, g, g, indexing="ij")).reshape(3, -1)
    vap = site + (rng.random(site.shape) - 0.5) * (2.0 * 0.25 * av)
    d = vap - L * np.rint(vap / L)                                         # from the nearest image of the corner
    vap = vap[:, np.sum(d * d, axis=0) > (R + 1.1) ** 2]                   # 1 sigma shell + the dense jitter
    return _finish(rng, L, np.concatenate([dense, vap], axis=1), rc_over_L)


def slab(L=SLAB_S, seed=202, rc_over_L=RC_OVER_L):
    """A dense slab (rho ~ 0.95, +-5 % jitter) 0.3 L thick across the x = 0 face, periodic in y and z; vacuum elsewhere."""
    rng = _rng(seed)
    m = int(round(L / 0.95 ** (-1.0 / 3.0)))
    a = L / m
    k = int(round(0.3 * L / a))
    gx = (np.arange(k, dtype=np.float64) + 0.5 - 0.5 * k) * a
    gy = (np.arange(m, dtype=np.float64) + 0.5) * a
    site = np.stack(np.meshgrid(gx, gy, gy, indexing="ij")).reshape(3, -1)
    r = site + (rng.random(site.shape) - 0.5) * (2.0 * 0.05 * a)
    return _finish(rng, L, r, rc_over_L)


def sheets(L=SHEETS_S, seed=303, rc_over_L=RC_OVER_L):
    """Two monolayers on jittered square lattices of spacing ~1.1, one at z = 0.0 exactly and one at z = L - 1.0: they
    are 1.0 apart through the face and every z is one of two doubles (tile boxes of zero width on that axis)."""
    rng = _rng(seed)
    m = int(round(L / 1.1))
    a = L / m
    g = (np.arange(m, dtype=np.float64) + 0.5) * a
    xy = np.stack(np.meshgrid(g, g, indexing="ij")).reshape(2, -1)
    layers = []
    for z in (0.0, L - 1.0):
        p = xy + (rng.random(xy.shape) - 0.5) * (2.0 * 0.05 * a)
        layers.append(np.concatenate([p, np.full((1, p.shape[1]), z)], axis=0))
    n = 2 * m * m
    r = np.concatenate(layers, axis=1)
    r[:2] = _wrap(r[:2], L)                              # z is left alone: 0.0 and L - 1.0 as written
    r = r[:, rng.permutation(n)]
    return init_params(n, L, DT, rc_over_L * L), np.ascontiguousarray(r), np.ascontiguousarray(_velocities(rng, n))


def raw_images(cfg, seed=404, lo=-0.69, hi=1.69):
    """The wrapped configuration with k L added per particle and axis, k in {-1, 0, +1} at random, k = 0 where the result
    would leave (lo L, hi L).  The array is used as it is, in fp64, by the engine and by the oracle."""
    p, r, v = cfg
    L = p.box_length
    rng = _rng(seed)
    k = rng.integers(-1, 2, size=r.shape).astype(np.float64)
    x = r + k * L
    x = np.where((x > lo * L) & (x < hi * L), x, r)
    return p, np.ascontiguousarray(x), v.copy()


# ---- checks shared by the CPU test and the GPU tests (numpy only) -------------------------------------------------

def pair_pass(r, L, rc, chunk=64):
    """One chunked O(n^2) minimum-image pass over the unordered pairs -> (minimum distance, sum of |4 (r^-12 - r^-6)| over
    the pairs inside rc).  Seconds at n = 20 000."""
    n = r.shape[1]
    invL, rc2 = 1.0 / L, rc * rc
    dmin2, sabs = np.inf, 0.0
    bd, bt, b2 = (np.empty(chunk * n) for _ in range(3))
    for i0 in range(0, n, chunk):
        i1 = min(i0 + chunk, n)
        shape = (i1 - i0, n - i0)                              # columns j >= i0 only: every unordered pair once
        d, t, r2 = (b[:shape[0] * shape[1]].reshape(shape) for b in (bd, bt, b2))
        r2[:] = 0.0
        for c in r:
            np.subtract(c[i0:i1, None], c[None, i0:], out=d)
            np.multiply(d, invL, out=t)
            np.rint(t, out=t)
            t *= L
            d -= t
            d *= d
            r2 += d
        r2[np.tril_indices(i1 - i0)] = np.inf                  # j <= i inside the diagonal block
        dmin2 = min(dmin2, r2.min())
        u = 1.0 / r2[r2 < rc2]
        u3 = u * u * u
        sabs += np.sum(np.abs(u3 * u3 - u3))
    return float(np.sqrt(dmin2)), 4.0 * sabs


def kd_tiles(r, tile=64):
    """A simple spatial sort: recursive median split along the longest extent down to `tile` particles -> index lists."""
    out, stack = [], [np.arange(r.shape[1])]
    while stack:
        idx = stack.pop()
        if len(idx) <= tile:
            out.append(idx)
            continue
        x = r[:, idx]
        ax = int(np.argmax(x.max(axis=1) - x.min(axis=1)))
        half = ((len(idx) + 2 * tile - 1) // (2 * tile)) * tile          # left half: a whole number of tiles
        order = idx[np.argsort(x[ax], kind="stable")]
        stack += [order[:half], order[half:]]
    return out


def tile_skip_fraction(r, L, rc, tile=64):
    """Fraction of the unordered pairs of distinct tiles whose boxes are further apart than rc under the minimum image."""
    rw = _wrap(r.copy(), L)
    tiles = kd_tiles(rw, tile)
    lo = np.array([rw[:, t].min(axis=1) for t in tiles])
    hi = np.array([rw[:, t].max(axis=1) for t in tiles])
    T = len(tiles)
    g2 = np.zeros((T, T))
    for ax in range(3):
        dlo = lo[:, None, ax] - hi[None, :, ax]                            # differences x_i - x_j lie in [dlo, dhi]
        dhi = hi[:, None, ax] - lo[None, :, ax]
        g = np.full((T, T), np.inf)
        for m in (-1, 0, 1):
            c = m * L
            g = np.minimum(g, np.where((dlo <= c) & (c <= dhi), 0.0, np.minimum(np.abs(dlo - c), np.abs(dhi - c))))
        g2 += g * g
    iu = np.triu_indices(T, 1)
    return float(np.mean(g2[iu] > rc * rc)), T
