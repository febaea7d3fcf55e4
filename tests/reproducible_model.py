"""CPU model of the reproducible mode (LJMD_PRECISION_FP64_REPRODUCIBLE, include/ljmd.h): the definition the GPU must
match bit for bit.  A helper module of the tests, not collected (no test_ prefix).

Per ordered pair (i, j), j != i, the reference's arithmetic (lj_potential_energy.f90:109-183): dnint minimum image,
r2 = (dx*dx + dy*dy) + dz*dz, r2 < rc2, u = 1/r2, u3 = (u*u)*u, u6 = u3*u3, m = 2*u6 - u3, fx = (m*dx)*u.  Every term t
enters an exact integer sum as Q(t) = RNE(t 2^64); each result is ONE correctly rounded conversion of an integer
(CPython's int / int is correctly rounded).  numpy never contracts a*b + c into an fma, so the terms are the reference's.
"""
from __future__ import annotations

import math

import numpy as np

SCALE = 2.0 ** 64
BOUND = 2.0 ** 40          # |t| < BOUND, else LJMD_ERR_RANGE
ROW_CHUNK = 256


class RangeError(ValueError):
    """A term was not finite or |t| >= 2^40: the GPU returns LJMD_ERR_RANGE."""


def dnint(x: np.ndarray) -> np.ndarray:
    """Fortran dnint / C round: half away from zero (np.round is half to even).  x - trunc(x) is exact."""
    t = np.trunc(x)
    f = x - t
    return t + np.where(np.abs(f) >= 0.5, np.sign(x), 0.0)


def q_limbs(t: np.ndarray, axis=None):
    """Q(t) = rint(t 2^64) split exactly into int64 limbs c2 2^64 + c1 2^32 + c0 (|c2| < 2^40, |c1|, |c0| < 2^32) and
    summed along `axis`: fewer than 2^23 terms cannot overflow an int64 limb sum."""
    v = np.rint(np.asarray(t, dtype=np.float64) * SCALE)      # t 2^64 is exact, rint is RNE
    c2 = np.trunc(v * 2.0 ** -64)
    r = v - c2 * SCALE                                          # |r| < 2^64, a multiple of ulp(v): exact
    c1 = np.trunc(r * 2.0 ** -32)
    c0 = r - c1 * 2.0 ** 32
    return tuple(np.sum(c.astype(np.int64), axis=axis) for c in (c2, c1, c0))


def limbs_to_int(c2, c1, c0) -> int:
    return (int(c2) << 64) + (int(c1) << 32) + int(c0)


def q_sum(t: np.ndarray) -> int:
    """sum of Q(t) over all elements, as an exact Python int"""
    return limbs_to_int(*q_limbs(np.ravel(t)))


def R(x: int) -> float:
    """RNE(x) 2^-64 for an exact integer x: ONE rounding"""
    return x / (1 << 64)


def check_range(*terms: np.ndarray) -> None:
    for t in terms:
        if t.size and not np.all(np.abs(t) < BOUND):        # NaN fails the test too
            raise RangeError("term not finite or |t| >= 2^40")


def tail_constants(n: int, L: float, rc: float):
    """lj_potential_energy.f90:205-223, the same expressions as ljmd_create"""
    npd = float(n)
    volume = L * L * L
    rc3 = (rc * rc) * rc
    rc6 = ((rc * rc) * (rc * rc)) * (rc * rc)
    tf = 8.0 * math.pi * (npd * npd) / (volume * rc3)
    return (tf * ((1.0 / (3.0 * rc6)) - 1.0) / 3.0, 2.0 * tf * (-2.0 / (3.0 * rc6) + 1.0),
            2.0 * tf * (26.0 / (3.0 * rc6) - 7.0))


def pair_sums(r: np.ndarray, L: float, rc: float):
    """r [3, n] -> (X, s12, s6): X[k][i] = sum_j Q(f_k ij) (Python ints), s12 / s6 = sums of Q(u6) / Q(u3) over the
    ORDERED pairs.  RangeError where the GPU fails."""
    x, y, z = (np.ascontiguousarray(r[k], dtype=np.float64) for k in range(3))
    n = x.size
    invL, rc2 = 1.0 / L, rc * rc
    X = [[0] * n for _ in range(3)]
    s12 = s6 = 0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for i0 in range(0, n, ROW_CHUNK):
            i1 = min(i0 + ROW_CHUNK, n)
            d = []
            for c in (x, y, z):
                d0 = c[i0:i1, None] - c[None, :]
                d.append(d0 - L * dnint(d0 * invL))
            dx, dy, dz = d
            r2 = dx * dx + dy * dy + dz * dz
            inside = r2 < rc2
            inside[np.arange(i1 - i0), np.arange(i0, i1)] = False       # j != i
            u = np.where(inside, 1.0 / np.where(inside, r2, 1.0), 0.0)
            u3 = u * u * u
            u6 = u3 * u3
            m = 2.0 * u6 - u3
            f = [np.where(inside, m * dk * u, 0.0) for dk in (dx, dy, dz)]
            check_range(*[fk[inside] for fk in f], u6[inside])
            for k in range(3):
                c2, c1, c0 = q_limbs(f[k], axis=1)
                for ii in range(i1 - i0):
                    X[k][i0 + ii] = limbs_to_int(c2[ii], c1[ii], c0[ii])
            s12 += q_sum(u6[inside])
            s6 += q_sum(u3[inside])
    return X, s12, s6


def forces(r: np.ndarray, L: float, rc: float, tail: bool = True):
    """r [3, n] -> (epot, d_epot, dd_epot, a [3, n]) of the contract; RangeError where the GPU fails."""
    X, s12, s6 = pair_sums(r, L, rc)
    acc = np.array([[24.0 * R(xi) for xi in Xk] for Xk in X]).reshape(3, -1)
    assert s12 % 2 == 0 and s6 % 2 == 0          # every unordered pair twice, with the same bits
    s12 //= 2
    s6 //= 2
    te, td, tdd = tail_constants(acc.shape[1], L, rc) if tail else (0.0, 0.0, 0.0)
    epot = 4.0 * R(s12 - s6) + te
    d_epot = 24.0 * R(s6 - 2 * s12) + td
    dd_epot = 24.0 * R(26 * s12 - 7 * s6) + tdd
    return epot, d_epot, dd_epot, acc


def kinetic(v: np.ndarray) -> float:
    """0.5 ((Kx + Ky) + Kz), Kx = R(sum_i Q(vx_i * vx_i))"""
    t = [np.asarray(v[k], dtype=np.float64) * np.asarray(v[k], dtype=np.float64) for k in range(3)]
    check_range(*t)
    kx, ky, kz = (R(q_sum(tk)) for tk in t)
    return 0.5 * ((kx + ky) + kz)


def run(r0: np.ndarray, v0: np.ndarray, L: float, dt: float, rc: float, nsteps: int, tail: bool = True):
    """t = 0 force call, then nsteps velocity-Verlet steps (verlet.f90:58-95, md_simulation_program.f90:339-353) as the
    GPU integrates them.  -> dict(r, ru, v, a final, scalars [nsteps, 4] = epot, ekin, d_epot, dd_epot per step,
    first = (epot, d_epot, dd_epot) of t = 0)."""
    r = np.array(r0, dtype=np.float64)
    ru = r.copy()
    v = np.array(v0, dtype=np.float64)
    invL, dt_half = 1.0 / L, 0.5 * dt
    dt_sq_half = dt_half * dt
    e, d, dd, a = forces(r, L, rc, tail)
    first = (e, d, dd)
    sc = np.empty((nsteps, 4))
    for s in range(nsteps):
        r1 = (r + v * dt) + a * dt_sq_half
        r1 = r1 - L * np.floor(r1 * invL)
        dr = r1 - r
        dr = dr - L * dnint(dr * invL)
        ru = ru + dr
        r = r1
        v = v + a * dt_half
        e, d, dd, a = forces(r, L, rc, tail)
        v = v + a * dt_half
        sc[s] = (e, kinetic(v), d, dd)
    return {"r": r, "ru": ru, "v": v, "a": a, "scalars": sc, "first": first}
