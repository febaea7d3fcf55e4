// ljmd_tcf.h -- MSD / VACF of the system resident on a one-rank engine (include/ljmd.h: ljmd_tcf_*): argument blocks of
// the three kernels of ljmd_tcf.hip.  The host side, with the sizes of their buffers, is ljmd_resident.h.
//
// Everything the feature stores is in PARTICLE-ID order (id = index in the arrays of the last ljmd_set_state), padded
// to n_pad = n rounded up to kTcfBlock: cur[6][n_pad] = ru xyz, v xyz of the current snapshot, ring[slots][6][n_pad] the
// stored origins.  Padding elements are zeroed at configure and never written: a padding "particle" yields the terms 0
// and 0, Q(0) = 0, so the terms kernel has no bounds test.  Only the gather kernel sees the slot permutation.
#ifndef LJMD_TCF_H
#define LJMD_TCF_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ljmdt {

constexpr int kTcfMaxLag = 4096;            // LJMD_TCF_MAX_LAG
constexpr int kTcfMaxOrigins = 512;         // LJMD_TCF_MAX_ORIGINS: ring slots = max_lag / stride + 1
constexpr int kTcfThreads = 256;            // threads of a workgroup of every kernel here
constexpr int kTcfK = 4;                    // particles a thread of the terms kernel owns: tid + k kTcfThreads
constexpr int kTcfBlock = kTcfThreads * kTcfK;   // particle ids per workgroup of the terms kernel
constexpr int kTcfTargetWorkgroups = 1024;  // the live origins are cut into slices until the grid has about this many
constexpr int kTcfMaxChunk = 128;           // live origins per slice at most: its LDS entries, one more for lag 0 ...
constexpr int kTcfLdsBudget = 8 * 1024;     // ... stay inside this many bytes (32 per entry)
static_assert((kTcfMaxChunk + 1) * 32 <= kTcfLdsBudget, "LDS budget of a slice's entries");
constexpr size_t kTcfMaxN = (size_t)1 << 23;   // largest system the sizes below are checked for (tests/tcf_host)

// The window of a snapshot (ljmd_tcf_host.h: TcfWindow): origin e = 0 .. n_live - 1 at lag lag_first - e stride in ring
// slot (slot_first + e) % slots; entry n_live is the lag-0 entry of the newest origin, present when that origin is at
// lag 1.  Slice y of the grid takes the origins [y chunk, min(n_live, (y + 1) chunk)); the last slice the lag-0 entry.

struct TcfGatherArgs {
    const double *ru, *v;   // [3][P] slot order
    const int *perm;        // [P] slot -> particle id (>= n on padding slots)
    double *cur;            // [6][n_pad] particle-id order
    double *store;          // the ring slot [6][n_pad] that takes this snapshot, or NULL
    int n, P;
    size_t n_pad;
};

struct TcfTermsArgs {
    const double *cur;              // [6][n_pad]
    const double *ring;             // [slots][6][n_pad]
    unsigned long long *part;       // [nblk][ents][2 kinds][2 words]: rows of block x, entries of slice y
    int32_t *flag;                  // [nblk][slots]: element (x, y) = 1 when a term of that workgroup was out of range
    size_t n_pad;
    int nblk, slots, ents, stride;  // ents = slots + 1: up to `slots` live origins and the lag-0 entry
    int n_live, lag_first, slot_first;
    int chunk, slices;
};

struct TcfFoldArgs {
    const unsigned long long *part;
    const int32_t *flag;
    uint64_t *sums;                 // [2][max_lag + 1][3] signed 192-bit: kind 0 = MSD, 1 = VACF
    int32_t *range;                 // sticky word
    int nblk, slots, ents, stride, max_lag;
    int n_live, lag_first;
    int chunk, slices;
};

hipError_t launch_tcf_gather(const TcfGatherArgs &a, hipStream_t s);
hipError_t launch_tcf_terms(const TcfTermsArgs &a, hipStream_t s);
hipError_t launch_tcf_fold(const TcfFoldArgs &a, hipStream_t s);

}  // namespace ljmdt
#endif
