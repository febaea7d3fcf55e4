"""TEST INFRASTRUCTURE: the density modes of include/ljmd.h (ljmd_rhok_*) restated in numpy fp64 arithmetic and Python
ints.  Every operation below is one IEEE double operation with its own rounding (numpy never fuses), in the order of the
definition; Q(t) = RNE(t 2^64) is split exactly into int64 limbs (reproducible_model.q_limbs) and the limbs are summed
over the particles as integers.  words(r, L, modes) is what ljmd_rhok_read_exact returns for the particles r [3, n];
doubles(words) what ljmd_rhok_read returns."""
from __future__ import annotations

import numpy as np

from reproducible_model import R, limbs_to_int, q_limbs

TWO_PI = float.fromhex("0x1.921fb54442d18p+2")
# the correctly rounded doubles of (-1)^j / (2j + 1)! from S15 down to S3, and of (-1)^j / (2j)! from C16 down to C2
S_COEFFS = [float.fromhex(h) for h in ("-0x1.ae7f3e733b81fp-41", "0x1.6124613a86d09p-33", "-0x1.ae64567f544e4p-26",
                                       "0x1.71de3a556c734p-19", "-0x1.a01a01a01a01ap-13", "0x1.1111111111111p-7",
                                       "-0x1.5555555555555p-3")]
C_COEFFS = [float.fromhex(h) for h in ("0x1.ae7f3e733b81fp-45", "-0x1.93974a8c07c9dp-37", "0x1.1eed8eff8d898p-29",
                                       "-0x1.27e4fb7789f5cp-22", "0x1.a01a01a01a01ap-16", "-0x1.6c16c16c16c17p-10",
                                       "0x1.5555555555555p-5", "-0x1p-1")]
MODE_CHUNK = 256        # modes per numpy pass: [chunk, n] temporaries


def turns(x, L: float):
    """t = x / L ; t - rint(t)"""
    t = np.asarray(x, dtype=np.float64) / np.float64(L)
    return t - np.rint(t)


def terms(t, modes):
    """t [3, n] turns, modes [m, 3] -> (C, S) [m, n]: the definition's cos and sin of every (mode, particle)"""
    nd = np.asarray(modes).astype(np.float64)
    phi = (nd[:, 0:1] * t[0][None, :] + nd[:, 1:2] * t[1][None, :]) + nd[:, 2:3] * t[2][None, :]
    f = phi - np.rint(phi)
    q = np.rint(4.0 * f)
    g = f - 0.25 * q
    th = g * TWO_PI
    zz = th * th
    ps = np.full_like(zz, S_COEFFS[0])
    for c in S_COEFFS[1:]:
        ps = ps * zz + c
    s = th + th * (zz * ps)
    pc = np.full_like(zz, C_COEFFS[0])
    for c in C_COEFFS[1:]:
        pc = pc * zz + c
    c = 1.0 + zz * pc
    k = np.where(np.isfinite(q), q, 0.0).astype(np.int64) & 3
    C = np.select([k == 0, k == 1, k == 2], [c, -s, -c], s)
    S = np.select([k == 0, k == 1, k == 2], [s, c, -s], -c)
    return C, S


def words(r, L: float, modes):
    """r [3, n] (the positions ljmd_get_state returns as r), modes [m, 3] -> ([[Re, Im] per mode] as Python ints, flag):
    the sums of Q(C) and Q(S) over the particles; a term that is not finite enters as two zeros and sets the flag."""
    r = np.asarray(r, dtype=np.float64)
    modes = np.asarray(modes).reshape(-1, 3)
    out, flag = [], False
    with np.errstate(all="ignore"):
        t = np.stack([turns(r[a], L) for a in range(3)])
        for m0 in range(0, modes.shape[0], MODE_CHUNK):
            C, S = terms(t, modes[m0:m0 + MODE_CHUNK])
            bad = ~(np.isfinite(C) & np.isfinite(S))
            flag = flag or bool(bad.any())
            C = np.where(bad, 0.0, C)
            S = np.where(bad, 0.0, S)
            re, im = q_limbs(C, axis=1), q_limbs(S, axis=1)
            for j in range(C.shape[0]):
                out.append([limbs_to_int(*(l[j] for l in re)), limbs_to_int(*(l[j] for l in im))])
    return out, flag


def doubles(w):
    """[[Re, Im] per mode] -> complex [m]: one rounding of each integer"""
    return np.array([complex(R(re), R(im)) for re, im in w], dtype=np.complex128)


def to_limbs(x: int):
    """a Python int as the three int64 limbs of a signed 192-bit integer, least significant first"""
    u = x & ((1 << 192) - 1)
    limbs = [(u >> (64 * k)) & ((1 << 64) - 1) for k in range(3)]
    return [v - (1 << 64) if v >= (1 << 63) else v for v in limbs]
