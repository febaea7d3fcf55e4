// ljmd_batch_rhok.h -- argument block and launcher of the batch engine's density modes kernel (ljmd_batch_rhok.hip),
// shared with its host side ljmd_rhok_batch.cpp (include/ljmd.h: ljmd_batch_rhok_*).  The device layout and the replica
// table are the batch engine's (ljmd_batch.h); the arithmetic of a term is ljmd_rhok_arith.h, the mode limits ljmd_rhok.h's.
#ifndef LJMD_BATCH_RHOK_H
#define LJMD_BATCH_RHOK_H

#include "ljmd_batch.h"
#include "ljmd_rhok.h"

namespace ljmdb {

constexpr int kBatchRhokMaxSnapshots = 262144;         // LJMD_BATCH_RHOK_MAX_SNAPSHOTS
constexpr int kBatchRhokMaxEntries = 1 << 24;          // LJMD_BATCH_RHOK_MAX_ENTRIES: max_snapshots * B * n_modes
constexpr int kBatchRhokMaxN = 4096;                   // LJMD_BATCH_MAX_N: a lane adds at most 4096 parts below 2^34
constexpr int kBatchRhokModeChunk = ljmdc::kRhokModeChunk;   // modes of a workgroup: one per lane
constexpr int kBatchRhokRowWords = ljmdc::kRhokRowWords;     // int64 words of one mode: Re[3], Im[3]
// waves of a workgroup, sharing the replica's tiles: 2, 4 or 8.  Measured (profiles/batch_rhok_rate.txt): with 1024
// replicas of 256 particles 4 and 8 waves agree within their spread and 2 are up to 13 % slower; with 64 replicas of
// 4096 particles 8 waves take 0.25 ms, 4 waves 0.28 ms and 2 waves 0.52 ms -- few workgroups, each with 64 tiles
constexpr int kBatchRhokWaves = 8;

// grid = (n_blocks table entries) x (ceil(n_modes / 64) mode chunks) workgroups of `waves` waves; workgroup (x, y) owns
// replica rep[g0 + x] and the modes 64 y .. 64 y + 63 of the list completely
struct BatchRhokArgs {
    const double *r;        // [3][plane]: the wrapped positions (planes rx ry rz of the state)
    const BatchReplica *rep;
    const int32_t *modes;   // [n_modes][3]
    uint64_t *words;        // [rows][B][n_modes][kBatchRhokRowWords] signed 192-bit, sample-major; row (row, b, mode) is
                            // written by one workgroup alone
    int32_t *range;         // [B] sticky: set to 1 when a term of replica b was not finite
    size_t plane;
    size_t B;               // replicas of the handle (row stride)
    int64_t row;            // snapshot this launch writes, 0 <= row < rows
    int64_t rows;           // snapshots the series holds
    int g0;
    int n_modes;
};

inline bool batch_rhok_ok(const BatchRhokArgs &a, int n_blocks, int waves)
{
    return a.r && a.rep && a.modes && a.words && a.range && a.n_modes >= 1 && a.n_modes <= ljmdc::kRhokMaxModes &&
           a.row >= 0 && a.row < a.rows && a.g0 >= 0 && n_blocks >= 1 && (size_t)a.g0 + (size_t)n_blocks <= a.B &&
           (waves == 2 || waves == 4 || waves == 8);
}

// one launch of n_blocks table entries of any kernel class: nothing here scales with the class's NMAX
hipError_t launch_batch_rhok(const BatchRhokArgs &a, int n_blocks, int waves, hipStream_t s);

}  // namespace ljmdb
#endif
