// ljmd_vanhove.h -- van Hove self-correlation G_s(r, tau) of the system resident on a one-rank engine (include/ljmd.h:
// ljmd_vanhove_*): argument blocks of the three kernels of ljmd_vanhove.hip.  The host side, with the sizes of their
// buffers, is ljmd_resident.h.
//
// The layout is that of ljmd_tcf.h without the velocities: everything is in PARTICLE-ID order (id = index in the arrays
// of the last ljmd_set_state), padded to n_pad = n rounded up to kVhBlock: cur[3][n_pad] = ru xyz of the current
// snapshot, ring[slots][3][n_pad] the stored origins.  Padding elements are zeroed at configure and never written: a
// padding "particle" yields r2 = r4 = 0, Q(0) = 0, so the sums need no bounds test; the histogram does (bin 0 would
// count it) and the terms kernel guards it by id < n.  Only the gather kernel sees the slot permutation.
#ifndef LJMD_VANHOVE_H
#define LJMD_VANHOVE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ljmdv {

constexpr int kVhMaxLag = 4096;             // LJMD_VANHOVE_MAX_LAG
constexpr int kVhMaxOrigins = 512;          // LJMD_VANHOVE_MAX_ORIGINS: ring slots = max_lag / stride + 1
constexpr int kVhMaxBins = 4096;            // LJMD_VANHOVE_MAX_BINS (the overflow column is one more)
constexpr int kVhThreads = 256;             // threads of a workgroup of every kernel here
constexpr int kVhK = 4;                     // particles a thread of the terms kernel owns: tid + k kVhThreads
constexpr int kVhBlock = kVhThreads * kVhK; // particle ids per workgroup of the terms kernel
constexpr int kVhTargetWorkgroups = 1024;   // the live origins are cut into slices until the grid has about this many
constexpr int kVhMaxChunk = 128;            // live origins per slice at most: its LDS entries, one more for lag 0 ...
constexpr int kVhLdsBudget = 24 * 1024;     // ... and the 32-bit histogram with its overflow column stay inside this
static_assert((kVhMaxChunk + 1) * 32 + (kVhMaxBins + 1) * 4 <= kVhLdsBudget, "LDS budget of a slice's entries and histogram");
constexpr size_t kVhMaxN = (size_t)1 << 23; // largest system the sizes are checked for (tests/vanhove_host)

// The window of a snapshot (ljmd_tcf_host.h: TcfWindow): origin e = 0 .. n_live - 1 at lag lag_first - e stride in ring
// slot (slot_first + e) % slots; entry n_live is the lag-0 entry of the newest origin, present when that origin is at
// lag 1.  Slice y of the grid takes the origins [y chunk, min(n_live, (y + 1) chunk)); the last slice the lag-0 entry.

struct VhGatherArgs {
    const double *ru;       // [3][P] slot order
    const int *perm;        // [P] slot -> particle id (>= n on padding slots)
    double *cur;            // [3][n_pad] particle-id order
    double *store;          // the ring slot [3][n_pad] that takes this snapshot, or NULL
    int n, P;
    size_t n_pad;
};

struct VhTermsArgs {
    const double *cur;              // [3][n_pad]
    const double *ring;             // [slots][3][n_pad]
    unsigned long long *hist;       // [max_lag + 1][nbins + 1]: column nbins = overflow
    unsigned long long *part;       // [nblk][ents][2 kinds][2 words]: rows of block x, entries of slice y; kind 0 = r2, 1 = r4
    int32_t *flag;                  // [nblk][slots]: element (x, y) = 1 when a term of that workgroup was out of range
    size_t n_pad;
    double dr, inv_dr;
    int n, nbins, max_lag;
    int nblk, slots, ents, stride;  // ents = slots + 1: up to `slots` live origins and the lag-0 entry
    int n_live, lag_first, slot_first;
    int chunk, slices;
};

struct VhFoldArgs {
    const unsigned long long *part;
    const int32_t *flag;
    uint64_t *sums;                 // [2][max_lag + 1][3] signed 192-bit: kind 0 = S2, 1 = S4
    int32_t *range;                 // sticky word
    int nblk, slots, ents, stride, max_lag;
    int n_live, lag_first;
    int chunk, slices;
};

hipError_t launch_vanhove_gather(const VhGatherArgs &a, hipStream_t s);
hipError_t launch_vanhove_terms(const VhTermsArgs &a, hipStream_t s);
hipError_t launch_vanhove_fold(const VhFoldArgs &a, hipStream_t s);

}  // namespace ljmdv
#endif
