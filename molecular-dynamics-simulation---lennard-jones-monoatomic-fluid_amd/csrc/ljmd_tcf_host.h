// ljmd_tcf_host.h -- the one copy of the host arithmetic of the MSD / VACF accumulation, shared by the batch engine
// (ljmd_batch_tcf.cpp) and the single engine (ljmd_tcf.cpp): which stored origins a snapshot meets, where it is stored
// itself, what it adds to the counts, and the quotient a sum becomes.  Host code only.
#ifndef LJMD_TCF_HOST_H
#define LJMD_TCF_HOST_H

#include "ljmd_internal.h"

#include <algorithm>
#include <cstdint>

namespace ljmdh {

// Snapshot s of a trajectory.  Its live origins are the multiples t0 of the stride with 1 <= s - t0 <= max_lag:
// origin e = 0 .. n_live - 1 is t0 = t0_first + e stride, at lag lag_first - e stride, in ring slot
// (slot_first + e) % slots.  n_live == 0 and store_slot < 0: the snapshot meets nothing and is not kept.
struct TcfWindow {
    int n_live = 0, lag_first = 0, slot_first = 0;
    int store_slot = -1;    // ring slot that takes this snapshot, or -1: not an origin
};

inline TcfWindow tcf_window(int64_t s, int max_lag, int stride_, int slots)
{
    const int64_t stride = stride_, lo = std::max<int64_t>(0, s - max_lag);
    const int64_t first = (lo + stride - 1) / stride * stride, last = s >= 1 ? (s - 1) / stride * stride : -1;
    TcfWindow w;
    if (last >= first) {
        w.n_live = (int)((last - first) / stride) + 1;
        w.lag_first = (int)(s - first);
        w.slot_first = (int)(first / stride % slots);
    }
    w.store_slot = s % stride == 0 ? (int)(s / stride % slots) : -1;
    return w;
}

// the host's share of one snapshot: every live origin counts at its lag, and the one at lag 1 at lag 0 too
inline void tcf_count(const TcfWindow &w, int stride, int64_t *counts /* [max_lag + 1] */)
{
    for (int e = 0; e < w.n_live; ++e) {
        const int lag = w.lag_first - e * stride;
        ++counts[lag];
        if (lag == 1) ++counts[0];
    }
}

// fixed(S) / ((double)n * (double)count), 0 for count == 0: one rounding of the integer, one division (n count < 2^53:
// the product is exact)
inline double tcf_quotient(const uint64_t (&x)[3], int32_t n, int64_t count)
{
    return count == 0 ? 0.0 : ljmdk::fixed_to_double(x) / ((double)n * (double)count);
}

}  // namespace ljmdh
#endif
