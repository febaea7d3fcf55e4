// ljmd_stress.h -- pressure tensor of the system resident on the single / sharded engine (include/ljmd.h:
// ljmd_stress_*): argument blocks of the three kernels of ljmd_stress.hip and the conversion of a snapshot's words.  The
// host side is ljmd_resident.h.
//
// The layout is the engine's (ljmd_internal.h): exchange buffer pos[G][3][P], velocities v[3][P] of the own block,
// 64-slot tiles, TB tiles per rank block, T = G TB tiles, NaN positions and zero velocities on the padding slots.
// The walk, its grid and the tile boxes it skips by are those of the resident g(r) (ljmd_rdf.h).
#ifndef LJMD_STRESS_H
#define LJMD_STRESS_H

#include "ljmd_internal.h"
#include "ljmd_rdf.h"
#include "ljmd_series.h"

namespace ljmds {

using ljmdr::kRdfBoxStride;
using ljmdr::kRdfWaves;

constexpr int kStressComponents = 6;            // xx, yy, zz, xy, xz, yz
constexpr int kStressWords = 2 * kStressComponents * 3;    // int64 words of one snapshot: K[6][3], then S[6][3]
constexpr int kStressMaxSnapshots = 262144;     // LJMD_STRESS_MAX_SNAPSHOTS
constexpr int kStressMaxN = 1 << 23;            // kFixedMaxN: a lane adds fewer than 2^23 terms below 2^104
constexpr int kStressKinThreads = 256;          // threads of a kinetic workgroup ...
constexpr int kStressKinPerThread = 8;          // ... and slots per thread
constexpr int kStressKinBlock = kStressKinThreads * kStressKinPerThread;
constexpr int kStressFoldWaves = 13;            // one wave per row of the fold: K[6], S[6], the tile-pair counts

// the walk of rdf_pairs_kernel (ljmd_rdf.h: RdfPairArgs), grid = (ceil(TB / kRdfWaves), ceil(U / chunk))
struct StressPairArgs {
    const double *pos;              // exchange buffer [G][3][P]
    const double *bbox;             // [T][kRdfBoxStride] from launch_rdf_boxes
    uint64_t *part;                 // [workgroups][6][3] sums of Q(term) of the workgroup; workgroup = y grid.x + x
    unsigned long long *pcount;     // [workgroups][2] tile pairs evaluated / considered
    unsigned *pflag;                // [workgroups] 1 = a pair of the workgroup was out of range
    int P, G, rank, TB, T;
    int U, chunk;
    int skip;                       // 0: every tile pair is evaluated (positions not known to be compact)
    double L, invL, rc2;
    double rc2_skin;                // rc^2 (1 + 1e-10): a tile pair is skipped only when its bound exceeds this
};

using StressKineticArgs = ljmdk::SeriesKineticArgs;      // kpart [blocks][6][3]
using StressFoldArgs = ljmdk::SeriesFoldArgs;            // row [kStressWords]

hipError_t launch_stress_pairs(const StressPairArgs &a, dim3 grid, hipStream_t s);
hipError_t launch_stress_kinetic(const StressKineticArgs &a, hipStream_t s);
hipError_t launch_stress_fold(const StressFoldArgs &a, hipStream_t s);

// p[c] = (R(K[c]) + 12 R(S[c])) / ((L L) L) of one snapshot's words (inline: the batch engine's read uses it too)
inline void stress_doubles(const int64_t *words, double L, double *out6)
{
    const double V = (L * L) * L;
    for (int c = 0; c < kStressComponents; ++c) {
        const int64_t *k = words + 3 * c, *s = words + 3 * (kStressComponents + c);
        const uint64_t kw[3] = {(uint64_t)k[0], (uint64_t)k[1], (uint64_t)k[2]};
        const uint64_t sw[3] = {(uint64_t)s[0], (uint64_t)s[1], (uint64_t)s[2]};
        out6[c] = (ljmdk::fixed_to_double(kw) + 12.0 * ljmdk::fixed_to_double(sw)) / V;
    }
}

}  // namespace ljmds
#endif
