// ljmd_batch_stress.h -- argument block and launcher of the batch engine's pressure tensor kernel
// (ljmd_batch_stress.hip), shared with its host side ljmd_stress_batch.cpp (include/ljmd.h: ljmd_batch_stress_*).
// The device layout and the replica table are the batch engine's (ljmd_batch.h).
#ifndef LJMD_BATCH_STRESS_H
#define LJMD_BATCH_STRESS_H

#include "ljmd_batch.h"

namespace ljmdb {

constexpr int kBatchStressMaxSnapshots = 262144;       // LJMD_BATCH_STRESS_MAX_SNAPSHOTS
constexpr int kBatchStressWords = 36;                  // int64 words of one (snapshot, replica): K[6][3], then S[6][3]

// One snapshot of every replica of a launch: the replica's resident wrapped r and v -> the 12 exact integer sums of
// ljmd_stress_* in row (row, b) of the series, the workgroup being that row's only writer.  Same launch geometry as
// launch_batch.
struct BatchStressArgs {
    const double *state;    // [12][plane]: r = planes 0..2, v = planes 6..8
    uint64_t *words;        // [rows][B][kBatchStressWords] signed 192-bit, sample-major
    int32_t *range;         // [B] sticky: set to 1 when a pair or a particle of replica b was out of range
    const BatchReplica *rep;
    size_t plane;
    size_t B;               // replicas of the handle (row stride)
    int64_t row;            // snapshot this launch writes, 0 <= row < rows
    int64_t rows;           // snapshots the series holds
    int g0;
};
hipError_t launch_batch_stress(const BatchStressArgs &a, int n_max, int n_blocks, hipStream_t s);

}  // namespace ljmdb
#endif
