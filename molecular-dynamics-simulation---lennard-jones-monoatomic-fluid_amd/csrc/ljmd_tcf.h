// ljmd_tcf.h -- MSD / VACF of the system resident on a one-rank engine (include/ljmd.h: ljmd_tcf_*): argument blocks of
// the three kernels of ljmd_tcf.hip.  Constants, layout (6 components per particle: ru xyz, v xyz), the gather and the
// fold block are those of the time-origin observables (ljmd_origins.h); the host side is ljmd_resident.h.
#ifndef LJMD_TCF_H
#define LJMD_TCF_H

#include "ljmd_origins.h"

namespace ljmdt {

constexpr int kTcfMaxLag = ljmdk::kOriginMaxLag;            // LJMD_TCF_MAX_LAG
constexpr int kTcfMaxOrigins = ljmdk::kOriginMaxOrigins;    // LJMD_TCF_MAX_ORIGINS
constexpr int kTcfThreads = ljmdk::kOriginThreads;
constexpr int kTcfK = ljmdk::kOriginK;
constexpr int kTcfBlock = ljmdk::kOriginBlock;
constexpr int kTcfTargetWorkgroups = ljmdk::kOriginTargetWorkgroups;
constexpr int kTcfMaxChunk = ljmdk::kOriginMaxChunk;
constexpr int kTcfLdsBudget = 8 * 1024;     // a slice's LDS entries, one more for lag 0, stay inside this many bytes
static_assert((kTcfMaxChunk + 1) * 32 <= kTcfLdsBudget, "LDS budget of a slice's entries");
constexpr size_t kTcfMaxN = ljmdk::kOriginMaxN;

using TcfGatherArgs = ljmdk::OriginGatherArgs;
using TcfFoldArgs = ljmdk::OriginFoldArgs;     // sums: kind 0 = MSD, 1 = VACF

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

hipError_t launch_tcf_gather(const TcfGatherArgs &a, hipStream_t s);
hipError_t launch_tcf_terms(const TcfTermsArgs &a, hipStream_t s);
hipError_t launch_tcf_fold(const TcfFoldArgs &a, hipStream_t s);

}  // namespace ljmdt
#endif
