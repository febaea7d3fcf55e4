// ljmd_heatflux.h -- heat flux of the system resident on the one-rank engine (include/ljmd.h: ljmd_heatflux_*):
// argument blocks of the three kernels of ljmd_heatflux.hip and the conversion of a snapshot's words.  The host side is
// ljmd_resident.h.
//
// The layout is the engine's (ljmd_internal.h) with G = 1: exchange buffer pos[3][P], velocities v[3][P] in the same
// slot order, 64-slot tiles, T tiles, NaN positions and zero velocities on the padding slots.  The walk, its grid and
// the tile boxes it skips by are those of the resident g(r) (ljmd_rdf.h), in the unordered form only.
#ifndef LJMD_HEATFLUX_H
#define LJMD_HEATFLUX_H

#include "ljmd_internal.h"
#include "ljmd_rdf.h"
#include "ljmd_series.h"

namespace ljmdq {

using ljmdr::kRdfBoxStride;
using ljmdr::kRdfWaves;

constexpr int kHeatfluxPairComponents = 6;      // P x, y, z, then C x, y, z: what the pair kernel sums
constexpr int kHeatfluxKinComponents = 3;       // E x, y, z: what the kinetic kernel sums
constexpr int kHeatfluxRows = kHeatfluxKinComponents + kHeatfluxPairComponents;    // E[3], P[3], C[3]
constexpr int kHeatfluxWords = kHeatfluxRows * 3;       // int64 words of one snapshot
constexpr int kHeatfluxMaxSnapshots = 262144;   // LJMD_HEATFLUX_MAX_SNAPSHOTS
constexpr int kHeatfluxMaxN = 1 << 23;          // kFixedMaxN: a lane adds fewer than 2^23 terms below 2^104
constexpr int kHeatfluxColumns = 4;             // columns per batch of the pair loop: position and velocity of each are
                                                // wave-uniform (12 SGPRs a column)
constexpr int kHeatfluxKinThreads = 256;        // threads of a kinetic workgroup ...
constexpr int kHeatfluxKinPerThread = 8;        // ... and slots per thread
constexpr int kHeatfluxKinBlock = kHeatfluxKinThreads * kHeatfluxKinPerThread;
constexpr int kHeatfluxFoldWaves = kHeatfluxRows + 1;   // one wave per row of the fold: E[3], P[3], C[3], the counts

// the unordered walk of rdf_pairs_kernel (ljmd_rdf.h: RdfPairArgs, G = 1), grid = (ceil(T / kRdfWaves), ceil(U / chunk))
struct HeatfluxPairArgs {
    const double *pos;              // exchange buffer [3][P]
    const double *vel;              // [3][P], the slot order of pos
    const double *bbox;             // [T][kRdfBoxStride] from launch_rdf_boxes
    uint64_t *part;                 // [workgroups][6][3] sums of Q(term) of the workgroup; workgroup = y grid.x + x
    unsigned long long *pcount;     // [workgroups][2] tile pairs evaluated / considered
    unsigned *pflag;                // [workgroups] 1 = a pair of the workgroup was out of range
    int P, T;
    int U, chunk;
    int skip;                       // 0: every tile pair is evaluated (positions not known to be compact)
    double L, invL, rc2;
    double rc2_skin;                // rc^2 (1 + 1e-10): a tile pair is skipped only when its bound exceeds this
};

using HeatfluxKineticArgs = ljmdk::SeriesKineticArgs;    // kpart [blocks][3][3]
using HeatfluxFoldArgs = ljmdk::SeriesFoldArgs;          // row [kHeatfluxWords]

hipError_t launch_heatflux_pairs(const HeatfluxPairArgs &a, dim3 grid, hipStream_t s);
hipError_t launch_heatflux_kinetic(const HeatfluxKineticArgs &a, hipStream_t s);
hipError_t launch_heatflux_fold(const HeatfluxFoldArgs &a, hipStream_t s);

// j[a] = (0.5 R(E[a]) + R(P[a]) + 6 R(C[a])) / ((L L) L) of one snapshot's words; parts9 (may be NULL) [3][3]: the three
// summands over V, convective, potential, collisional
inline void heatflux_doubles(const int64_t *words, double L, double *j3, double *parts9)
{
    const double V = (L * L) * L;
    for (int a = 0; a < 3; ++a) {
        double r[3];
        for (int p = 0; p < 3; ++p) {
            const int64_t *w = words + 3 * (3 * p + a);
            const uint64_t u[3] = {(uint64_t)w[0], (uint64_t)w[1], (uint64_t)w[2]};
            r[p] = ljmdk::fixed_to_double(u);
        }
        const double e = 0.5 * r[0], c = 6.0 * r[2];
        if (j3) j3[a] = (e + r[1] + c) / V;
        if (parts9) {
            parts9[a] = e / V;
            parts9[3 + a] = r[1] / V;
            parts9[6 + a] = c / V;
        }
    }
}

}  // namespace ljmdq
#endif
