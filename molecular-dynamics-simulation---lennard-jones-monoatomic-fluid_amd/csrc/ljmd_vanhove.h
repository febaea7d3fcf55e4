// ljmd_vanhove.h -- van Hove self-correlation G_s(r, tau) of the system resident on a one-rank engine (include/ljmd.h:
// ljmd_vanhove_*): argument blocks of the three kernels of ljmd_vanhove.hip.  Constants, layout (3 components per
// particle: ru xyz), the gather and the fold block are those of the time-origin observables (ljmd_origins.h); the host
// side is ljmd_resident.h.  A padding "particle" yields r2 = r4 = 0, so the sums need no bounds test; the histogram does
// (bin 0 would count it) and the terms kernel guards it by id < n.
#ifndef LJMD_VANHOVE_H
#define LJMD_VANHOVE_H

#include "ljmd_origins.h"

namespace ljmdv {

constexpr int kVhMaxLag = ljmdk::kOriginMaxLag;             // LJMD_VANHOVE_MAX_LAG
constexpr int kVhMaxOrigins = ljmdk::kOriginMaxOrigins;     // LJMD_VANHOVE_MAX_ORIGINS
constexpr int kVhMaxBins = 4096;            // LJMD_VANHOVE_MAX_BINS (the overflow column is one more)
constexpr int kVhThreads = ljmdk::kOriginThreads;
constexpr int kVhK = ljmdk::kOriginK;
constexpr int kVhBlock = ljmdk::kOriginBlock;
constexpr int kVhTargetWorkgroups = ljmdk::kOriginTargetWorkgroups;
constexpr int kVhMaxChunk = ljmdk::kOriginMaxChunk;
constexpr int kVhLdsBudget = 24 * 1024;     // a slice's LDS entries and the 32-bit histogram with its overflow column
static_assert((kVhMaxChunk + 1) * 32 + (kVhMaxBins + 1) * 4 <= kVhLdsBudget, "LDS budget of a slice's entries and histogram");
constexpr size_t kVhMaxN = ljmdk::kOriginMaxN;

using VhGatherArgs = ljmdk::OriginGatherArgs;  // v is not read: NULL
using VhFoldArgs = ljmdk::OriginFoldArgs;      // sums: kind 0 = S2, 1 = S4

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

hipError_t launch_vanhove_gather(const VhGatherArgs &a, hipStream_t s);
hipError_t launch_vanhove_terms(const VhTermsArgs &a, hipStream_t s);
hipError_t launch_vanhove_fold(const VhFoldArgs &a, hipStream_t s);

}  // namespace ljmdv
#endif
