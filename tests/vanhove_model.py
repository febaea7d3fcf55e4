"""CPU model of the engine's van Hove self-correlation (ljmd_vanhove_*, include/ljmd.h): the definition the GPU must
match integer for integer.  A helper module of the tests, not collected (no test_ prefix).

Snapshots s = 0, 1, 2, ... (ru [3, n]).  When snapshot s arrives, every stored origin t0 with 1 <= s - t0 <= max_lag
contributes, per particle, d = ru(s) - ru(t0), r2 = (dx*dx + dy*dy) + dz*dz, r4 = r2 * r2, r = sqrt(r2), bin =
int(r / dr) -- H[s - t0][min(bin, nbins)] += 1, S2[s - t0] += Q(r2), S4[s - t0] += Q(r4) -- and, at s - t0 == 1, its
lag-0 row (d = ru(t0) - ru(t0)); then s is stored as an origin when s % origin_stride == 0.  A particle whose r4 is not
finite or >= 2^40 counts in the overflow column, enters both sums as 0 and sets the range flag.  numpy never contracts
a*b + c into an fma and its sqrt and division are correctly rounded; Q(t) = RNE(t 2^64) summed as Python ints
(reproducible_model.q_limbs); the results ONE rounding of the integer and one division."""
from __future__ import annotations

import numpy as np

from reproducible_model import BOUND, R, limbs_to_int, q_limbs

S2, S4 = 0, 1


class VanHoveModel:
    def __init__(self, max_lag: int, stride: int, nbins: int, rmax: float):
        assert 1 <= max_lag and stride >= 1 and nbins >= 1 and rmax > 0.0
        self.max_lag, self.stride, self.nbins, self.rmax = max_lag, stride, nbins, float(rmax)
        self.dr = self.rmax / nbins
        self.reset()

    def reset(self) -> None:
        self.H = np.zeros((self.max_lag + 1, self.nbins + 1), dtype=np.uint64)
        self.S = [[0] * (self.max_lag + 1) for _ in range(2)]     # exact Python ints: S2, S4
        self.counts = np.zeros(self.max_lag + 1, dtype=np.int64)
        self.range_flag = False
        self.new_trajectory()

    def new_trajectory(self) -> None:
        """what ljmd_set_state does: the origins are dropped, the numbering restarts, histogram, sums and counts stay"""
        self.s = 0
        self.origins = {}                                          # t0 -> ru

    def _add(self, lag: int, cur: np.ndarray, org: np.ndarray) -> None:
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            d = cur - org
            r2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
            r4 = r2 * r2
            ok = np.abs(r4) < BOUND                                # NaN and inf fail the test; r2 not finite -> r4 neither
            if not np.all(ok):
                self.range_flag = True
            r2 = np.where(ok, r2, 0.0)
            r4 = np.where(ok, r4, 0.0)
            q = np.sqrt(r2) / self.dr
            inside = ok & (q < self.nbins)
            bins = np.where(inside, np.floor(np.where(inside, q, 0.0)), self.nbins).astype(np.int64)
        self.H[lag] += np.bincount(bins, minlength=self.nbins + 1).astype(np.uint64)
        self.S[S2][lag] += limbs_to_int(*q_limbs(r2))
        self.S[S4][lag] += limbs_to_int(*q_limbs(r4))
        self.counts[lag] += 1

    def push(self, ru: np.ndarray) -> None:
        ru = np.array(ru, dtype=np.float64).reshape(3, -1)
        s = self.s
        live = [t0 for t0 in sorted(self.origins) if 1 <= s - t0 <= self.max_lag]
        for t0 in live:
            self._add(s - t0, ru, self.origins[t0])
        if live and live[-1] == s - 1:                             # the lag-0 row of the origin one snapshot back
            self._add(0, self.origins[s - 1], self.origins[s - 1])
        if s % self.stride == 0:
            self.origins[s] = ru
            for t0 in [t for t in self.origins if s + 1 - t > self.max_lag]:
                del self.origins[t0]
        self.s = s + 1

    def result(self, kind: int, n: int) -> np.ndarray:
        """[max_lag + 1]: R(S) / (n count), 0 where count == 0"""
        return np.array([R(self.S[kind][l]) / (n * int(c)) if c else 0.0 for l, c in enumerate(self.counts)])
