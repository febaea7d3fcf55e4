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

// One snapshot of every replica of a launch: the replica's resident wrapped r and v -> the 9 exact integer sums of
// ljmd_heatflux_* in row (row, b) of the series, the workgroup being that row's only writer.  Same launch geometry as
// launch_batch.
struct BatchHeatfluxArgs {
    const double *state;    // [12][plane]: r = planes 0..2, v = planes 6..8
    uint64_t *words;        // [rows][B][kBatchHeatfluxWords] signed 192-bit, sample-major
    int32_t *range;         // [B] sticky: set to 1 when a pair or a particle of replica b was out of range
    const BatchReplica *rep;
    size_t plane;
    size_t B;               // replicas of the handle (row stride)
    int64_t row;            // snapshot this launch writes, 0 <= row < rows
    int64_t rows;           // snapshots the series holds
    int g0;
};
hipError_t launch_batch_heatflux(const BatchHeatfluxArgs &a, int n_max, int n_blocks, hipStream_t s);

}  // namespace ljmdb
#endif
