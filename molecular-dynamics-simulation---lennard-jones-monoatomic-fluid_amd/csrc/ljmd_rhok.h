// ljmd_rhok.h -- density modes rho_k = sum_j exp(i k . r_j) of the system resident on the one-rank engine
// (include/ljmd.h: ljmd_rhok_*): constants, the grid of one accumulate, and the argument blocks of the two kernels of
// ljmd_rhok.hip.  The arithmetic of a term is ljmd_rhok_arith.h, the host side ljmd_resident.h.
//
// The layout is the engine's (ljmd_internal.h) with G = 1: exchange buffer pos[3][P], 64-slot tiles, T tiles, the
// device's slot -> id permutation perm[P]; a slot is live when its id lies in [0, n), every other slot is padding.
#ifndef LJMD_RHOK_H
#define LJMD_RHOK_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "ljmd_internal.h"

namespace ljmdc {

constexpr int kRhokMaxModes = 4096;             // LJMD_RHOK_MAX_MODES
constexpr int kRhokMaxIndex = 1023;             // LJMD_RHOK_MAX_INDEX
constexpr int kRhokMaxSnapshots = 262144;       // LJMD_RHOK_MAX_SNAPSHOTS
constexpr int kRhokMaxEntries = 1 << 24;        // LJMD_RHOK_MAX_ENTRIES
constexpr int kRhokMaxN = 1 << 23;              // kFixedMaxN: a lane adds fewer than 2^29 parts below 2^34
constexpr int kRhokModeChunk = 64;              // modes of a wave: one per lane
constexpr int kRhokWaves = 4;                   // waves of a workgroup of the terms kernel, each a unit of its own
constexpr int kRhokMaxChunks = 1024;            // particle chunks at most: rows of partials the fold adds per mode
constexpr int kRhokTargetUnits = 8192;          // waves that fill the card: 256 CUs x 4 SIMDs x 8
constexpr int kRhokFoldWaves = 8;               // waves of a fold workgroup, each adding every 8th row
constexpr int kRhokRowWords = 6;                // int64 words of one mode: Re[3], Im[3]

// the grid of one accumulate: mchunks chunks of 64 modes, pchunks chunks of `tiles` 64-slot tiles; a unit = one wave =
// (particle chunk, mode chunk)
struct RhokPlan {
    int mchunks = 0, pchunks = 0, tiles = 0;
};

// as many units as fill the card, no particle chunk empty, at most kRhokMaxChunks of them
inline RhokPlan rhok_plan(int T, int n_modes)
{
    RhokPlan p;
    p.mchunks = (n_modes + kRhokModeChunk - 1) / kRhokModeChunk;
    int want = (kRhokTargetUnits + p.mchunks - 1) / p.mchunks;
    if (want > kRhokMaxChunks) want = kRhokMaxChunks;
    if (want > T) want = T;
    p.tiles = (T + want - 1) / want;
    p.pchunks = (T + p.tiles - 1) / p.tiles;
    return p;
}

// grid = ceil(pchunks mchunks / kRhokWaves) workgroups of kRhokWaves waves; unit u: mode chunk u % mchunks, particle
// chunk u / mchunks
struct RhokTermsArgs {
    const double *pos;              // exchange buffer [3][P]
    const int *perm;                // [P] slot -> id
    const int32_t *modes;           // [n_modes][3]
    uint64_t *part;                 // [pchunks][mchunks 64][kRhokRowWords]: sums of Q(C), Q(S) of the chunk's live slots
    unsigned *flag;                 // [pchunks][mchunks] 1 = a term of the unit was out of range
    int P, T, n, n_modes;
    int mchunks, pchunks, tiles;
    double L;
};

// grid = mchunks workgroups of kRhokFoldWaves waves; lane = mode
struct RhokFoldArgs {
    const uint64_t *part;
    const unsigned *flag;
    int n_modes, mchunks, pchunks;
    uint64_t *row;                  // [n_modes][kRhokRowWords] of the series: this launch is its only writer
    int32_t *range;                 // sticky
};

inline bool rhok_terms_ok(const RhokTermsArgs &a)
{
    return a.pos && a.perm && a.modes && a.part && a.flag && a.T >= 1 && (long long)a.P >= (long long)a.T * 64 && a.n >= 1 &&
           a.n <= kRhokMaxN && a.n_modes >= 1 && a.n_modes <= kRhokMaxModes && a.tiles >= 1 && a.pchunks >= 1 &&
           a.pchunks <= kRhokMaxChunks && a.mchunks == (a.n_modes + kRhokModeChunk - 1) / kRhokModeChunk &&
           (long long)a.pchunks * a.tiles >= a.T && (long long)(a.pchunks - 1) * a.tiles < a.T;
}

inline bool rhok_fold_ok(const RhokFoldArgs &a)
{
    return a.part && a.flag && a.row && a.range && a.n_modes >= 1 && a.n_modes <= kRhokMaxModes && a.pchunks >= 1 &&
           a.pchunks <= kRhokMaxChunks && a.mchunks == (a.n_modes + kRhokModeChunk - 1) / kRhokModeChunk;
}

// the doubles of ljmd_rhok_read and ljmd_batch_rhok_read: `count` signed 192-bit integers of three limbs each -> one
// correctly rounded conversion of each
inline void rhok_doubles(const int64_t *words, size_t count, double *rho)
{
    for (size_t k = 0; k < count; ++k) {
        const uint64_t u[3] = {(uint64_t)words[3 * k], (uint64_t)words[3 * k + 1], (uint64_t)words[3 * k + 2]};
        rho[k] = ljmdk::fixed_to_double(u);
    }
}

hipError_t launch_rhok_terms(const RhokTermsArgs &a, hipStream_t s);
hipError_t launch_rhok_fold(const RhokFoldArgs &a, hipStream_t s);

}  // namespace ljmdc
#endif
