// ljmd_batch_heatflux.h -- argument block and launcher of the batch engine's heat flux kernel
// (ljmd_batch_heatflux.hip), shared with its host side ljmd_heatflux_batch.cpp (include/ljmd.h: ljmd_batch_heatflux_*).
// The device layout and the replica table are the batch engine's (ljmd_batch.h).
#ifndef LJMD_BATCH_HEATFLUX_H
#define LJMD_BATCH_HEATFLUX_H

#include "ljmd_batch.h"

namespace ljmdb {

constexpr int kBatchHeatfluxMaxSnapshots = 262144;     // LJMD_BATCH_HEATFLUX_MAX_SNAPSHOTS
constexpr int kBatchHeatfluxRows = 9;                  // E[3], P[3], C[3]
constexpr int kBatchHeatfluxWords = 27;                // int64 words of one (snapshot, replica): [9][3]
constexpr int kBatchHeatfluxChunk = 2048;              // column particles whose r and v sit in LDS at a time

// BatchSeriesArgs (ljmd_batch.h) with words [rows][B][kBatchHeatfluxWords]: the 9 exact integer sums of ljmd_heatflux_* per replica.
using BatchHeatfluxArgs = BatchSeriesArgs;
hipError_t launch_batch_heatflux(const BatchHeatfluxArgs &a, int n_max, int n_blocks, hipStream_t s);

}  // namespace ljmdb
#endif
