// ljmd_batch_stress.h -- argument block and launcher of the batch engine's pressure tensor kernel
// (ljmd_batch_stress.hip), shared with its host side ljmd_stress_batch.cpp (include/ljmd.h: ljmd_batch_stress_*).
// The device layout and the replica table are the batch engine's (ljmd_batch.h).
#ifndef LJMD_BATCH_STRESS_H
#define LJMD_BATCH_STRESS_H

#include "ljmd_batch.h"

namespace ljmdb {

constexpr int kBatchStressMaxSnapshots = 262144;       // LJMD_BATCH_STRESS_MAX_SNAPSHOTS
constexpr int kBatchStressWords = 36;                  // int64 words of one (snapshot, replica): K[6][3], then S[6][3]

// BatchSeriesArgs (ljmd_batch.h) with words [rows][B][kBatchStressWords]: the 12 exact integer sums of ljmd_stress_* per replica.
using BatchStressArgs = BatchSeriesArgs;
hipError_t launch_batch_stress(const BatchStressArgs &a, int n_max, int n_blocks, hipStream_t s);

}  // namespace ljmdb
#endif
