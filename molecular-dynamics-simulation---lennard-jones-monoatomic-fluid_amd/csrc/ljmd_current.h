// ljmd_current.h -- current modes j_k = sum_j v_j exp(i k . r_j) of the system resident on the one-rank engine
// (include/ljmd.h: ljmd_current_*): constants and the argument blocks of the two kernels of ljmd_current.hip.  The
// arithmetic of a term is ljmd_current_arith.h over ljmd_rhok_arith.h, the host side ljmd_resident.h.  The mode list,
// its limits and the grid of one accumulate (RhokPlan, rhok_plan) are those of the density modes (ljmd_rhok.h).
//
// The layout is the engine's (ljmd_internal.h) with G = 1: exchange buffer pos[3][P] and velocities v[3][P] in the same
// slot order, 64-slot tiles, T tiles, the device's slot -> id permutation perm[P]; a slot is live when its id lies in
// [0, n), every other slot is padding.
#ifndef LJMD_CURRENT_H
#define LJMD_CURRENT_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "ljmd_internal.h"
#include "ljmd_rhok.h"

namespace ljmdc {

constexpr int kCurrentMaxSnapshots = 262144;    // LJMD_CURRENT_MAX_SNAPSHOTS
constexpr int kCurrentMaxEntries = 1 << 22;     // LJMD_CURRENT_MAX_ENTRIES
constexpr int kCurrentSums = 6;                 // sums of one mode: x Re, x Im, y Re, y Im, z Re, z Im
constexpr int kCurrentRowWords = 3 * kCurrentSums;      // int64 words of one mode
constexpr int kCurrentWaves = 4;                // waves of a workgroup of the terms kernel, each a unit of its own
// waves of a fold workgroup, each adding every 4th row.  With the 8 of the density modes' fold the LDS in which the
// waves meet would be 18 words x 64 lanes x 8 waves = 73 728 bytes, above the 64 KiB of static LDS; 4 waves need 36 864
// and still read every row of partials once, whole (144 contiguous bytes per lane), where a fold of the components in
// turn would launch or loop three times over strided thirds of a row.  The fold is a small part of an accumulate.
constexpr int kCurrentFoldWaves = 4;

// grid = ceil(pchunks mchunks / kCurrentWaves) workgroups of kCurrentWaves waves; unit u: mode chunk u % mchunks,
// particle chunk u / mchunks
struct CurrentTermsArgs {
    const double *pos;              // exchange buffer [3][P]
    const double *v;                // [3][P]
    const int *perm;                // [P] slot -> id
    const int32_t *modes;           // [n_modes][3]
    uint64_t *part;                 // [pchunks][mchunks 64][kCurrentRowWords]: the six sums of the chunk's live slots
    unsigned *flag;                 // [pchunks][mchunks] 1 = a term of the unit was out of range
    int P, T, n, n_modes;
    int mchunks, pchunks, tiles;
    double L;
};

// grid = mchunks workgroups of kCurrentFoldWaves waves; lane = mode
struct CurrentFoldArgs {
    const uint64_t *part;
    const unsigned *flag;
    int n_modes, mchunks, pchunks;
    uint64_t *row;                  // [n_modes][kCurrentRowWords] of the series: this launch is its only writer
    int32_t *range;                 // sticky
};

inline bool current_terms_ok(const CurrentTermsArgs &a)
{
    return a.pos && a.v && a.perm && a.modes && a.part && a.flag && a.T >= 1 && (long long)a.P >= (long long)a.T * 64 &&
           a.n >= 1 && a.n <= kRhokMaxN && a.n_modes >= 1 && a.n_modes <= kRhokMaxModes && a.tiles >= 1 && a.pchunks >= 1 &&
           a.pchunks <= kRhokMaxChunks && a.mchunks == (a.n_modes + kRhokModeChunk - 1) / kRhokModeChunk &&
           (long long)a.pchunks * a.tiles >= a.T && (long long)(a.pchunks - 1) * a.tiles < a.T;
}

inline bool current_fold_ok(const CurrentFoldArgs &a)
{
    return a.part && a.flag && a.row && a.range && a.n_modes >= 1 && a.n_modes <= kRhokMaxModes && a.pchunks >= 1 &&
           a.pchunks <= kRhokMaxChunks && a.mchunks == (a.n_modes + kRhokModeChunk - 1) / kRhokModeChunk;
}

hipError_t launch_current_terms(const CurrentTermsArgs &a, hipStream_t s);
hipError_t launch_current_fold(const CurrentFoldArgs &a, hipStream_t s);

}  // namespace ljmdc
#endif
