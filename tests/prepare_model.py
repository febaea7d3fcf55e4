"""CPU model of ljmd_batch_prepare (include/ljmd.h): the definition the GPU must match, in numpy and Python ints.  A
helper module of the tests, not collected (no test_ prefix).

Per replica (n = 4 k^3, L), the steps of the reference's initial-configuration program
(scripts/md_initial_config_program.f90:58-121): a. FCC lattice, b. velocities from the reference's generator, c. centre
of mass removed with the exact integer sum of the reproducible mode, d. scaled to the target total energy; the warm-up
is reproducible_model.run.  numpy never contracts a*b + c into an fma, so the expressions are the reference's.
"""
from __future__ import annotations

import math

import numpy as np

import reproducible_model as M

MODULUS = 4_000_000
SEED_OFFSET = 1618033
TO_UNIT = 1.0 / 4.0e6          # `fac`: the rounded reciprocal, multiplied -- not a division by 4e6


def ran3_states(seed: int, count: int) -> np.ndarray:
    """the integer states of `count` draws of random_uniform (fortran/random_numbers.f90) after its first call with
    seed -|seed| has set the table up -- an integer restatement: every value of that module is an integer < 4e6"""
    table = [0] * 56                                   # 1-based, as the module's
    cur = abs(SEED_OFFSET - abs(int(seed))) % MODULUS
    table[55] = cur
    nxt = 1
    for i in range(1, 55):
        pos = (21 * i) % 55
        table[pos] = nxt
        nxt = cur - nxt
        if nxt < 0:
            nxt += MODULUS
        cur = table[pos]
    for _ in range(4):
        for i in range(1, 56):
            table[i] -= table[1 + (i + 30) % 55]
            if table[i] < 0:
                table[i] += MODULUS
    head, tail = 0, 31
    out = np.empty(count, dtype=np.int64)
    for j in range(count):
        head = head + 1 if head < 55 else 1
        tail = tail + 1 if tail < 55 else 1
        cur = table[head] - table[tail]
        if cur < 0:
            cur += MODULUS
        table[head] = cur
        out[j] = cur
    return out


def ran3(seed: int, count: int) -> np.ndarray:
    """`count` draws in [0, 1): double(m) * (1 / 4e6)"""
    return ran3_states(seed, count).astype(np.float64) * TO_UNIT


def cells_of(n: int) -> int:
    k = round((n / 4.0) ** (1.0 / 3.0))
    if 4 * k ** 3 != n:
        raise ValueError(f"n = {n} is not 4 k^3")
    return k


def lattice(n: int, L: float) -> np.ndarray:
    """-> r [3, n]: cells ix > iy > iz, four basis particles per cell (md_initial_config_program.f90:132-187)"""
    k = cells_of(n)
    a = np.float64(L) / np.float64(k)
    idx = np.arange(k, dtype=np.float64)
    ix, iy, iz = (g.ravel() for g in np.meshgrid(idx, idx, idx, indexing="ij"))
    x0, y0, z0 = ix * a, iy * a, iz * a
    h = np.float64(0.5) * a
    r = np.empty((3, k ** 3, 4))
    r[0] = np.stack([x0, x0, x0 + h, x0 + h], axis=1)
    r[1] = np.stack([y0, y0 + h, y0, y0 + h], axis=1)
    r[2] = np.stack([z0, z0 + h, z0 + h, z0], axis=1)
    return np.ascontiguousarray(r.reshape(3, n))


def velocities(n: int, seed: int) -> np.ndarray:
    """-> v [3, n] before the scaling: draws 3 i, 3 i + 1, 3 i + 2 minus 0.5, then v_cm = R(sum Q(v)) / dble(n) off"""
    v = (ran3(seed, 3 * n) - 0.5).reshape(n, 3).T.copy()
    for ax in range(3):
        v[ax] = v[ax] - M.R(M.q_sum(v[ax])) / float(n)
    return v


def scale_factor(target: float, epot0: float, ekin0: float) -> float:
    return math.sqrt((float(target) - float(epot0)) / float(ekin0))


def prepare(n: int, L: float, rc: float, seed: int, target: float, tail: bool = True) -> dict:
    """steps a-d in the reproducible mode -> dict(r, v0 (before the scaling), v, a, epot0, ekin0)"""
    r = lattice(n, L)
    v0 = velocities(n, seed)
    epot0, _, _, a = M.forces(r, L, rc, tail)
    ekin0 = M.kinetic(v0)
    v = v0 * scale_factor(target, epot0, ekin0)
    return {"r": r, "v0": v0, "v": v, "a": a, "epot0": epot0, "ekin0": ekin0}
