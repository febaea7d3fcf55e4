// ljmd_origins.h -- what the kernels of the engine's resident time-origin observables, MSD / VACF (ljmd_tcf.h) and the van
// Hove self-correlation (ljmd_vanhove.h), share with their host side: the constants of their grid, the layout of their
// buffers, and the argument blocks of the gather and the fold kernel.  The kernels' shared code is ljmd_origins_dev.h,
// the host core ljmd_origins.cpp.
//
// Everything an observable stores is in PARTICLE-ID order (id = index in the arrays of the last ljmd_set_state), padded
// to n_pad = n rounded up to kOriginBlock, with C components per particle (6: ru xyz, v xyz; 3: ru xyz alone):
// cur[C][n_pad] is the current snapshot, ring[slots][C][n_pad] the stored origins.  Padding elements are zeroed at
// configure and never written: a padding "particle" yields terms of 0, Q(0) = 0, so the sums need no bounds test.  Only
// the gather kernel sees the slot permutation.
//
// The window of a snapshot (ljmd_tcf_host.h: TcfWindow): origin e = 0 .. n_live - 1 at lag lag_first - e stride in ring
// slot (slot_first + e) % slots; entry n_live is the lag-0 entry of the newest origin, present when that origin is at
// lag 1.  Slice y of the grid takes the origins [y chunk, min(n_live, (y + 1) chunk)); the last slice the lag-0 entry.
#ifndef LJMD_ORIGINS_H
#define LJMD_ORIGINS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ljmdk {

constexpr int kOriginMaxLag = 4096;         // LJMD_TCF_MAX_LAG, LJMD_VANHOVE_MAX_LAG
constexpr int kOriginMaxOrigins = 512;      // LJMD_*_MAX_ORIGINS: ring slots = max_lag / stride + 1
constexpr int kOriginThreads = 256;         // threads of a workgroup of every kernel
constexpr int kOriginK = 4;                 // particles a thread of a terms kernel owns: tid + k kOriginThreads
constexpr int kOriginBlock = kOriginThreads * kOriginK;   // particle ids per workgroup of a terms kernel
constexpr int kOriginTargetWorkgroups = 1024;   // the live origins are cut into slices until the grid has about this many
constexpr int kOriginMaxChunk = 128;        // live origins per slice at most: its LDS entries (32 bytes), one more for lag 0
constexpr size_t kOriginMaxN = (size_t)1 << 23;   // largest system the sizes are checked for (tests/tcf_host, vanhove_host)

struct OriginGatherArgs {
    const double *ru, *v;   // [3][P] slot order; v is read for 6 components only
    const int *perm;        // [P] slot -> particle id (>= n on padding slots)
    double *cur;            // [C][n_pad] particle-id order
    double *store;          // the ring slot [C][n_pad] that takes this snapshot, or NULL
    int n, P;
    size_t n_pad;
};

struct OriginFoldArgs {
    const unsigned long long *part; // [nblk][ents][2 kinds][2 words]: rows of block x, entries of slice y
    const int32_t *flag;            // [nblk][slots]: element (x, y) = 1 when a term of that workgroup was out of range
    uint64_t *sums;                 // [2][max_lag + 1][3] signed 192-bit, one row per kind and lag
    int32_t *range;                 // sticky word
    int nblk, slots, ents, stride, max_lag;
    int n_live, lag_first;
    int chunk, slices;
};

inline bool origin_gather_ok(const OriginGatherArgs &a, bool with_v)
{
    return a.ru && (a.v || !with_v) && a.perm && a.cur && a.n >= 1 && a.P >= a.n && a.n_pad >= (size_t)a.n &&
           a.n_pad % kOriginBlock == 0;
}

// the checks the terms and the fold launch make of a window and its slices
inline bool origin_window_ok(int nblk, int slots, int ents, int stride, int max_lag, int n_live, int lag_first, int chunk,
                             int slices)
{
    return nblk >= 1 && slots >= 1 && slots <= kOriginMaxOrigins && ents == slots + 1 && stride >= 1 && max_lag >= 1 &&
           max_lag <= kOriginMaxLag && n_live >= 1 && n_live <= slots && lag_first <= max_lag &&
           lag_first - (n_live - 1) * stride >= 1 && chunk >= 1 && chunk <= kOriginMaxChunk && slices >= 1 && slices <= slots &&
           (long long)slices * chunk >= n_live && (long long)(slices - 1) * chunk < n_live;
}

inline bool origin_fold_ok(const OriginFoldArgs &a)
{
    return a.part && a.flag && a.sums && a.range &&
           origin_window_ok(a.nblk, a.slots, a.ents, a.stride, a.max_lag, a.n_live, a.lag_first, a.chunk, a.slices);
}

}  // namespace ljmdk
#endif
