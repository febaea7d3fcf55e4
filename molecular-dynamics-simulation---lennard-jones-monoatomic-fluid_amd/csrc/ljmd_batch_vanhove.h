// ljmd_batch_vanhove.h -- argument block and launcher of the batch engine's van Hove kernel (ljmd_batch_vanhove.hip),
// shared with its host side ljmd_vanhove_batch.cpp (include/ljmd.h: ljmd_batch_vanhove_*).  The device layout, the
// replica table and the common block of the time-origin observables -- snapshots, origins, window -- are ljmd_batch.h's.
#ifndef LJMD_BATCH_VANHOVE_H
#define LJMD_BATCH_VANHOVE_H

#include "ljmd_batch.h"

namespace ljmdb {

constexpr int kBatchVanhoveMaxLag = 4096;              // LJMD_BATCH_VANHOVE_MAX_LAG
constexpr int kBatchVanhoveMaxOrigins = 512;           // LJMD_BATCH_VANHOVE_MAX_ORIGINS: ring slots = max_lag / stride + 1
constexpr int kBatchVanhoveMaxBins = 1024;             // LJMD_BATCH_VANHOVE_MAX_BINS: 4100 bytes of LDS bins beside the entries

// BatchOriginArgs with a ring of ru alone (3 planes per slot) and kind 0 = S2, 1 = S4; per replica b, live origin and
// particle the bin of |ru(s) - ru(t0)| is counted in H[b][lag][.] beside Q(r2) and Q(r4) in the replica's rows of sums.
struct BatchVanhoveArgs : BatchOriginArgs {
    unsigned long long *hist;  // [B][max_lag + 1][nbins + 1]: replica b's rows are written by its workgroup alone
    const double *dr;       // [B] rmax[b] / nbins
    const double *inv_dr;   // [B] 1 / dr[b]
    int nbins;
};
hipError_t launch_batch_vanhove(const BatchVanhoveArgs &a, int n_max, int n_blocks, hipStream_t s);

}  // namespace ljmdb
#endif
