"""CPU model of the batch engine's MSD / VACF accumulation (ljmd_batch_tcf_*, include/ljmd.h): the definition the GPU
must match integer for integer.  A helper module of the tests, not collected (no test_ prefix).

Snapshots s = 0, 1, 2, ... of one replica (ru [3, n], v [3, n]).  When snapshot s arrives, every stored origin t0 with
1 <= s - t0 <= max_lag contributes sum_i Q(term_i) to S[kind][s - t0] (and, at s - t0 == 1, its lag-0 terms to
S[kind][0]); then s is stored as an origin when s % origin_stride == 0.  The terms are the reference's numpy expressions
(scripts/md_one_run_analysis.py:404-489; numpy never contracts a*b + c into an fma), Q(t) = RNE(t 2^64) summed as Python
ints (reproducible_model.q_limbs), the results ONE rounding of the integer and one division."""
from __future__ import annotations

import numpy as np

from reproducible_model import BOUND, R, limbs_to_int, q_limbs

MSD, VACF = 0, 1


def reference_counts(n_snap: int, max_lag: int, origin_stride: int) -> np.ndarray:
    """origins per lag of compute_*_tau_timeorig for n_snap snapshots (md_one_run_analysis.py:423-437)"""
    counts = np.zeros(max_lag + 1, dtype=np.int64)
    for t0 in range(0, n_snap - 1, origin_stride):
        lag = min(max_lag, (n_snap - 1) - t0)
        if lag > 0:
            counts[:lag + 1] += 1
    return counts


class TcfModel:
    def __init__(self, max_lag: int, origin_stride: int = 1):
        assert 1 <= max_lag and origin_stride >= 1
        self.max_lag, self.stride = max_lag, origin_stride
        self.reset()

    def reset(self) -> None:
        self.S = [[0] * (self.max_lag + 1) for _ in range(2)]     # exact Python ints
        self.counts = np.zeros(self.max_lag + 1, dtype=np.int64)
        self.range_flag = False
        self.new_trajectory()

    def new_trajectory(self) -> None:
        """what ljmd_batch_set_state does: the origins are dropped, the numbering restarts, the sums stay"""
        self.s = 0
        self.origins = {}                                          # t0 -> (ru, v)

    def _sums(self, t: np.ndarray):
        """t [m, n] -> m Python ints: sum_i Q(t[k, i]), an out-of-range term entering as 0"""
        ok = np.abs(t) < BOUND                                     # NaN fails the test too
        if not np.all(ok):
            self.range_flag = True
            t = np.where(ok, t, 0.0)
        c2, c1, c0 = q_limbs(t, axis=1)
        return [limbs_to_int(c2[k], c1[k], c0[k]) for k in range(t.shape[0])]

    def push(self, ru: np.ndarray, v: np.ndarray) -> None:
        ru = np.array(ru, dtype=np.float64).reshape(3, -1)
        v = np.array(v, dtype=np.float64).reshape(3, -1)
        s = self.s
        live = [t0 for t0 in sorted(self.origins) if 1 <= s - t0 <= self.max_lag]
        if live:                                                   # vectorised over the live origins
            o_ru = np.stack([self.origins[t0][0] for t0 in live])  # [m, 3, n]
            o_v = np.stack([self.origins[t0][1] for t0 in live])
            with np.errstate(over="ignore", invalid="ignore"):
                d = ru[None] - o_ru
                msd = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
                vacf = (v[None, 0] * o_v[:, 0] + v[None, 1] * o_v[:, 1]) + v[None, 2] * o_v[:, 2]
                for kind, t in ((MSD, msd), (VACF, vacf)):
                    for t0, q in zip(live, self._sums(t)):
                        self.S[kind][s - t0] += q
                for t0 in live:
                    self.counts[s - t0] += 1
                if live[-1] == s - 1:                              # the lag-0 terms of the origin one snapshot back
                    r0, v0 = self.origins[s - 1]
                    d0 = r0 - r0
                    self.S[MSD][0] += self._sums(((d0[0] * d0[0] + d0[1] * d0[1]) + d0[2] * d0[2])[None])[0]
                    self.S[VACF][0] += self._sums(((v0[0] * v0[0] + v0[1] * v0[1]) + v0[2] * v0[2])[None])[0]
                    self.counts[0] += 1
        if s % self.stride == 0:
            self.origins[s] = (ru, v)
            for t0 in [t for t in self.origins if s + 1 - t > self.max_lag]:
                del self.origins[t0]
        self.s = s + 1

    def result(self, kind: int, n: int) -> np.ndarray:
        """[max_lag + 1]: R(S) / (n count), 0 where count == 0"""
        return np.array([R(self.S[kind][l]) / (n * int(c)) if c else 0.0 for l, c in enumerate(self.counts)])
