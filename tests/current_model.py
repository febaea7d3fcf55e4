"""TEST INFRASTRUCTURE: the current modes of include/ljmd.h (ljmd_current_*) restated in numpy fp64 arithmetic and Python
ints, on top of the density modes' model (rhok_model.turns / terms): per (mode, particle) the six products v_a C and
v_a S, each one IEEE double product (numpy never fuses), the range rule, and Q(t) = RNE(t 2^64) split exactly into int64
limbs (reproducible_model.q_limbs) and summed over the particles as integers.  words(r, v, L, modes) is what
ljmd_current_read_exact returns for the particles r, v [3, n]; doubles(words) what ljmd_current_read returns."""
from __future__ import annotations

import numpy as np

import rhok_model
from reproducible_model import BOUND, R, limbs_to_int, q_limbs

MODE_CHUNK = 256        # modes per numpy pass: [chunk, n] temporaries


def products(v, C, S):
    """v [3, n], (C, S) [m, n] -> (t [6][m, n] in the order x Re, x Im, y Re, y Im, z Re, z Im, bad [m, n]): the six
    products, and where the whole term is out of range -- C or S not finite, or a product not finite or >= 2^40"""
    v = np.asarray(v, dtype=np.float64)
    t = []
    for a in range(3):
        t.append(v[a][None, :] * C)
        t.append(v[a][None, :] * S)
    bad = ~(np.isfinite(C) & np.isfinite(S))
    for p in t:
        bad |= ~(np.abs(p) < BOUND)             # NaN fails the comparison too
    return t, bad


def words(r, v, L: float, modes):
    """r, v [3, n] (what ljmd_get_state returns as r and v), modes [m, 3] -> ([[[Re, Im] per a = x, y, z] per mode] as
    Python ints, flag): the sums of Q(v_a C) and Q(v_a S) over the particles; a (particle, mode) term that is out of range
    enters all six sums as zero and sets the flag."""
    r = np.asarray(r, dtype=np.float64)
    modes = np.asarray(modes).reshape(-1, 3)
    out, flag = [], False
    with np.errstate(all="ignore"):
        t = np.stack([rhok_model.turns(r[a], L) for a in range(3)])
        for m0 in range(0, modes.shape[0], MODE_CHUNK):
            C, S = rhok_model.terms(t, modes[m0:m0 + MODE_CHUNK])
            prod, bad = products(v, C, S)
            flag = flag or bool(bad.any())
            limbs = [q_limbs(np.where(bad, 0.0, p), axis=1) for p in prod]
            for j in range(C.shape[0]):
                six = [limbs_to_int(*(l[j] for l in limbs[k])) for k in range(6)]
                out.append([[six[0], six[1]], [six[2], six[3]], [six[4], six[5]]])
    return out, flag


def doubles(w):
    """[[[Re, Im] x 3] per mode] -> complex [m, 3]: one rounding of each integer"""
    return np.array([[complex(R(re), R(im)) for re, im in mode] for mode in w], dtype=np.complex128).reshape(-1, 3)


def to_words(w):
    """[[[Re, Im] x 3] per mode] -> int64 [m, 3, 2, 3]: the limbs ljmd_current_read_exact returns"""
    return np.array([[[rhok_model.to_limbs(x) for x in pair] for pair in mode] for mode in w], dtype=np.int64).reshape(-1, 3, 2, 3)
