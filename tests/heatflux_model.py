"""CPU model of the resident heat flux (ljmd_heatflux_*, include/ljmd.h): the definition the GPU must match integer for
integer.  A helper module of the tests, not collected (no test_ prefix).

One snapshot is E[3], P[3], C[3] with axes x, y, z.  E[a] = sum over particles of Q(k2 v_a), k2 = vx*vx + vy*vy + vz*vz.
P[a] and C[a] = sums over the ORDERED pairs i != j with r2 < rc2 of Q(phi w_a) and Q(g d_a), with the pressure tensor's
pair arithmetic (stress_model.virial_words: dnint minimum image, r2 = (dx*dx + dy*dy) + dz*dz, u = 1/r2, u3 = (u*u)*u,
u6 = u3*u3, m = 2*u6 - u3, fx = (m*dx)*u) and w = v_i + v_j, phi = u6 - u3, g = (fx*wx + fy*wy) + fz*wz.  Q(t) =
RNE(t 2^64), summed as Python ints.  A pair whose fx, fy, fz, u6, wx, wy, wz, g or one of whose six terms is not finite
or has |t| >= 2^40 enters as six zeros and sets the range flag; a particle's k2 and three terms likewise.  numpy never
contracts a*b + c into an fma, so the terms are the definition's."""
from __future__ import annotations

import math

import numpy as np

from reproducible_model import BOUND, R, dnint, limbs_to_int, q_limbs

ROWS = ("Ex", "Ey", "Ez", "Px", "Py", "Pz", "Cx", "Cy", "Cz")
ROW_CHUNK = 256


def _sum_terms(terms, guards):
    """terms: arrays of one shape; guards: further arrays that must be in range.  -> (one Python int per term, flag, ok):
    the sums of Q(term) over the elements where every term and guard is in range, whether one was not, and the mask"""
    ok = np.ones(terms[0].shape, dtype=bool)
    for t in list(terms) + list(guards):
        ok &= np.abs(t) < BOUND                                    # NaN and inf fail the test too
    out = []
    for t in terms:
        c2, c1, c0 = q_limbs(np.where(ok, t, 0.0).ravel())
        out.append(limbs_to_int(c2, c1, c0))
    return out, not bool(np.all(ok)), ok


def kinetic_words(v):
    """v [3, m] -> (E[3] Python ints, range flag)"""
    v = np.asarray(v, dtype=np.float64).reshape(3, -1)
    with np.errstate(over="ignore", invalid="ignore"):
        k2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2]
        out, bad, _ = _sum_terms([k2 * v[0], k2 * v[1], k2 * v[2]], [k2])
    return out, bad


def pair_words(r, v, L: float, rc: float, want_stats: bool = True):
    """r, v [3, n] -> (P[3] + C[3] Python ints over the ordered pairs, range flag, stats).  stats, over the ordered pairs
    that entered: 'pairs' their number; 'phi' the sum of u6 - u3 (math.fsum); 'abs_P'[a] the sum of |phi w_a|;
    'abs_C'[a] the sum of (|fx wx| + |fy wy| + |fz wz|) |d_a|, which bounds every intermediate of g d_a.  With
    want_stats=False they are not formed (None): the integers and the flag do not depend on them."""
    x, y, z = (np.ascontiguousarray(r[k], dtype=np.float64) for k in range(3))
    vv = [np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(3, -1)[k]) for k in range(3)]
    n = x.size
    invL, rc2 = 1.0 / L, rc * rc
    S = [0] * 6
    flag = False
    pairs = 0
    phis, abs_p, abs_c = [], [[], [], []], [[], [], []]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for k0 in range(0, n, ROW_CHUNK):
            ii = np.arange(k0, min(n, k0 + ROW_CHUNK))
            d = []
            for c in (x, y, z):
                d0 = c[ii, None] - c[None, :]
                d.append(d0 - L * dnint(d0 * invL))
            r2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
            inside = r2 < rc2
            inside[np.arange(ii.size), ii] = False                 # j != i
            pi, pj = np.nonzero(inside)
            dd = [dk[pi, pj] for dk in d]
            w = [c[ii[pi]] + c[pj] for c in vv]
            u = 1.0 / r2[pi, pj]
            u3 = u * u * u
            u6 = u3 * u3
            m = 2.0 * u6 - u3
            f = [m * dk * u for dk in dd]
            phi = u6 - u3
            g = f[0] * w[0] + f[1] * w[1] + f[2] * w[2]
            terms = [phi * w[0], phi * w[1], phi * w[2], g * dd[0], g * dd[1], g * dd[2]]
            sums, bad, ok = _sum_terms(terms, f + [u6] + w + [g])
            S = [a + b for a, b in zip(S, sums)]
            flag = flag or bad
            if not want_stats:
                continue
            pairs += int(np.count_nonzero(ok))
            phis.append(math.fsum(phi[ok]))
            gabs = np.abs(f[0] * w[0]) + np.abs(f[1] * w[1]) + np.abs(f[2] * w[2])
            for a in range(3):
                abs_p[a].append(math.fsum(np.abs(terms[a][ok])))
                abs_c[a].append(math.fsum((gabs * np.abs(dd[a]))[ok]))
    if not want_stats:
        return S, flag, None
    stats = {"pairs": pairs, "phi": math.fsum(phis), "abs_P": [math.fsum(t) for t in abs_p],
             "abs_C": [math.fsum(t) for t in abs_c]}
    return S, flag, stats


def words(r, v, L: float, rc: float):
    """one snapshot -> (E[3] + P[3] + C[3] as a list of 9 Python ints, range flag)"""
    E, kbad = kinetic_words(v)
    S, sbad, _ = pair_words(r, v, L, rc, want_stats=False)
    return E + S, kbad or sbad


def to_limbs(x: int):
    """a signed 192-bit integer as three int64 limbs, least significant first (two's complement)"""
    u = x & ((1 << 192) - 1)
    limbs = [(u >> (64 * k)) & ((1 << 64) - 1) for k in range(3)]
    return [l - (1 << 64) if l >> 63 else l for l in limbs]


def doubles(w, L: float):
    """9 Python ints -> (j[3], parts[3, 3]): j[a] = (0.5 R(E[a]) + R(P[a]) + 6 R(C[a])) / ((L L) L) and its three
    summands over V (convective, potential, collisional), the arithmetic of ljmd_heatflux_from_exact"""
    V = (L * L) * L
    j = np.empty(3)
    parts = np.empty((3, 3))
    for a in range(3):
        e, p, c = 0.5 * R(w[a]), R(w[3 + a]), 6.0 * R(w[6 + a])
        j[a] = (e + p + c) / V
        parts[0, a], parts[1, a], parts[2, a] = e / V, p / V, c / V
    return j, parts
