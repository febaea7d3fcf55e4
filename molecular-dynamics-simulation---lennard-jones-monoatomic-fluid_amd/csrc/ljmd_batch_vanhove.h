// ljmd_batch_vanhove.h -- argument block and launcher of the batch engine's van Hove kernel (ljmd_batch_vanhove.hip),
// shared with its host side ljmd_vanhove_batch.cpp (include/ljmd.h: ljmd_batch_vanhove_*).  The device layout and the
// replica table are the batch engine's (ljmd_batch.h); snapshots, origins and the window are those of BatchTcfArgs.
#ifndef LJMD_BATCH_VANHOVE_H
#define LJMD_BATCH_VANHOVE_H

#include "ljmd_batch.h"

namespace ljmdb {

constexpr int kBatchVanhoveMaxLag = 4096;              // LJMD_BATCH_VANHOVE_MAX_LAG
constexpr int kBatchVanhoveMaxOrigins = 512;           // LJMD_BATCH_VANHOVE_MAX_ORIGINS: ring slots = max_lag / stride + 1
constexpr int kBatchVanhoveMaxBins = 1024;             // LJMD_BATCH_VANHOVE_MAX_BINS: 4100 bytes of LDS bins beside the entries

// One snapshot -- every replica's resident ru -- against the live origins of the ring: per replica b, live origin and
// particle the bin of |ru(s) - ru(t0)| counted in H[b][lag][.], Q(r2) and Q(r4) added to the replica's rows of sums; the
// snapshot is then stored as an origin when its number is a multiple of the origin stride.  Same launch geometry as
// launch_batch.  Origin e = 0 .. n_live - 1 is at lag lag_first - e * stride (1 <= lag <= max_lag), in ring slot
// (slot_first + e) % slots; when the newest origin is at lag 1 its lag-0 row is added too.
struct BatchVanhoveArgs {
    const double *state;    // [12][plane]: ru = planes 3..5
    double *ring;           // [slots][3][plane]: ru of the stored origins
    unsigned long long *hist;  // [B][max_lag + 1][nbins + 1]: replica b's rows are written by its workgroup alone
    uint64_t *sums;         // [B][2][max_lag + 1][3] signed 192-bit: kind 0 = S2, 1 = S4; likewise
    int32_t *range;         // [B] sticky: set to 1 when a term of replica b was out of range
    const double *dr;       // [B] rmax[b] / nbins
    const double *inv_dr;   // [B] 1 / dr[b]
    const BatchReplica *rep;
    size_t plane;
    int g0;
    int nbins;
    int max_lag, stride, slots;
    int n_live, lag_first, slot_first;
    int store_slot;         // ring slot that takes this snapshot, or -1: not an origin
};
hipError_t launch_batch_vanhove(const BatchVanhoveArgs &a, int n_max, int n_blocks, hipStream_t s);

}  // namespace ljmdb
#endif
