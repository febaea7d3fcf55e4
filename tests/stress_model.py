"""CPU model of the resident pressure tensor (ljmd_stress_*, include/ljmd.h): the definition the GPU must match integer
for integer.  A helper module of the tests, not collected (no test_ prefix).

Components xx, yy, zz, xy, xz, yz.  K[c] = sum over particles of Q(v_a v_b); S[c] = sum over the ORDERED pairs i != j with
r2 < rc2 of Q(f_a d_b), with the reproducible pair kernel's arithmetic (reproducible_model.pair_sums: dnint minimum
image, r2 = (dx*dx + dy*dy) + dz*dz, u = 1/r2, u3 = (u*u)*u, u6 = u3*u3, m = 2*u6 - u3, fx = (m*dx)*u).  Q(t) =
RNE(t 2^64), summed as Python ints.  A pair whose fx, fy, fz, u6 or one of whose six products is not finite or has
|t| >= 2^40 enters as six zeros and sets the range flag; a particle's six velocity products likewise.  numpy never
contracts a*b + c into an fma, so the terms are the definition's."""
from __future__ import annotations

import numpy as np

from reproducible_model import BOUND, R, dnint, limbs_to_int, q_limbs

COMPONENTS = ("xx", "yy", "zz", "xy", "xz", "yz")
ROW_CHUNK = 256


def _six(a, b):
    """the six products a_x b_x, a_y b_y, a_z b_z, a_x b_y, a_x b_z, a_y b_z"""
    return [a[0] * b[0], a[1] * b[1], a[2] * b[2], a[0] * b[1], a[0] * b[2], a[1] * b[2]]


def _sum_six(terms, guards):
    """terms: six arrays of one shape; guards: further arrays that must be in range.  -> (six Python ints, flag): the sums
    of Q(term) over the elements where every term and guard is in range, and whether one was not"""
    ok = np.ones(terms[0].shape, dtype=bool)
    for t in list(terms) + list(guards):
        ok &= np.abs(t) < BOUND                                    # NaN and inf fail the test too
    out = []
    for t in terms:
        c2, c1, c0 = q_limbs(np.where(ok, t, 0.0).ravel())
        out.append(limbs_to_int(c2, c1, c0))
    return out, not bool(np.all(ok))


def kinetic_words(v):
    """v [3, m] -> (K[6] Python ints, range flag)"""
    v = np.asarray(v, dtype=np.float64).reshape(3, -1)
    with np.errstate(over="ignore", invalid="ignore"):
        return _sum_six(_six(v, v), [])


def virial_words(r, L: float, rc: float, rows=None):
    """r [3, n] -> (S[6] Python ints over the ordered pairs (i in rows, j != i), range flag, sum over those ordered pairs
    of |2 u^6 - u^3|).  rows = None: all particles."""
    x, y, z = (np.ascontiguousarray(r[k], dtype=np.float64) for k in range(3))
    n = x.size
    rows = np.arange(n) if rows is None else np.asarray(rows)
    invL, rc2 = 1.0 / L, rc * rc
    S = [0] * 6
    flag = False
    mdu_abs = 0.0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for k0 in range(0, rows.size, ROW_CHUNK):
            ii = rows[k0:k0 + ROW_CHUNK]
            d = []
            for c in (x, y, z):
                d0 = c[ii, None] - c[None, :]
                d.append(d0 - L * dnint(d0 * invL))
            r2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
            inside = r2 < rc2
            inside[np.arange(ii.size), ii] = False                 # j != i
            pi, pj = np.nonzero(inside)
            dd = [dk[pi, pj] for dk in d]
            u = 1.0 / r2[pi, pj]
            u3 = u * u * u
            u6 = u3 * u3
            m = 2.0 * u6 - u3
            f = [m * dk * u for dk in dd]
            sums, bad = _sum_six(_six(f, dd), f + [u6])
            S = [a + b for a, b in zip(S, sums)]
            flag = flag or bad
            mdu_abs += float(np.sum(np.abs(m[np.isfinite(m)])))
    return S, flag, mdu_abs


def words(r, v, L: float, rc: float, rows=None):
    """one snapshot (or, with rows, the partial of a rank that owns those particles) -> (K[6] + S[6] as a list of 12
    Python ints, range flag)"""
    v = np.asarray(v, dtype=np.float64).reshape(3, -1)
    K, kbad = kinetic_words(v if rows is None else v[:, np.asarray(rows)])
    S, sbad, _ = virial_words(r, L, rc, rows)
    return K + S, kbad or sbad


def to_limbs(x: int):
    """a signed 192-bit integer as three int64 limbs, least significant first (two's complement)"""
    u = x & ((1 << 192) - 1)
    limbs = [(u >> (64 * k)) & ((1 << 64) - 1) for k in range(3)]
    return [l - (1 << 64) if l >> 63 else l for l in limbs]


def doubles(w, L: float):
    """12 Python ints -> p[6] = (R(K) + 12 R(S)) / ((L L) L), the arithmetic of ljmd_stress_from_exact"""
    V = (L * L) * L
    return np.array([(R(w[c]) + 12.0 * R(w[6 + c])) / V for c in range(6)])
