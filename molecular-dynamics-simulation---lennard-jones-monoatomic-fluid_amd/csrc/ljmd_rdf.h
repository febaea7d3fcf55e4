// ljmd_rdf.h -- g(r) of the system resident on the single / sharded engine (include/ljmd.h: ljmd_rdf_*): argument
// blocks of the two kernels of ljmd_rdf.hip, the tile-pair bound they skip by, and the tile walk itself (rdf_walk_tiles),
// which the pair kernels of the pressure tensor and the heat flux share.  The host side is ljmd_resident.h.
//
// The layout is the engine's (ljmd_internal.h): exchange buffer pos[G][3][P], 64-slot tiles, TB tiles per rank block,
// T = G TB tiles, NaN on the padding slots.
#ifndef LJMD_RDF_H
#define LJMD_RDF_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ljmdr {

constexpr int kRdfMaxBins = 8192;           // LJMD_RDF_MAX_BINS: 32 KiB of 32-bit LDS bins per workgroup
constexpr int kRdfWaves = 4;                // row tiles (waves) per workgroup: they share one LDS histogram
constexpr int kRdfBoxStride = 6;            // doubles per tile box: lo xyz, hi xyz
constexpr int kRdfTargetWorkgroups = 4096;  // the column walk is cut into slices until the grid has about this many
// Steps (column tiles) of one slice at most.  One workgroup adds to a 32-bit LDS bin, between zeroing and its flush,
// at most kRdfWaves x 64 rows x 64 columns x weight 2 per step = 2^15: 2^16 steps stay below 2^32 (rdf_lds_bound).
constexpr int kRdfMaxChunk = 65536;

// the most one workgroup can add to one LDS bin in one launch
constexpr uint64_t rdf_lds_bound(int chunk, int weight) { return (uint64_t)kRdfWaves * 64u * 64u * (uint64_t)weight * (uint64_t)chunk; }

struct RdfBoxArgs {
    const double *pos;      // exchange buffer [G][3][P]
    double *bbox;           // [T][kRdfBoxStride] exact boxes of the tiles; an all-padding tile gets lo = +inf, hi = -inf
    int P, TB, T;
};

// The walk.  Row tiles = the TB tiles of the own block; row tile I (global index rank TB + Il) takes the steps u of
// [0, U):   G == 1:  U = T / 2 + 1, column tile J = (I + u) mod T, weight 2 -- every unordered tile pair once (the tie
//                    u = T / 2 of an even T from I < T / 2 only), inside the diagonal tile the pairs j > i;
//           G  > 1:  U = T, J = u, weight 1 -- own rows x all columns, the self pair left out by index.
// grid = (ceil(TB / kRdfWaves), ceil(U / chunk)).
struct RdfPairArgs {
    const double *pos;
    const double *bbox;
    unsigned long long *hist;       // [nbins], added to
    unsigned long long *count;      // [2] tile pairs evaluated / considered, added to
    int P, G, rank, TB, T;
    int U, chunk;
    int nbins;
    int skip;                       // 0: every tile pair is evaluated (positions not known to be compact)
    double L, invL, rmax, dr, inv_dr;
    double rmax2_skin;              // rmax^2 (1 + 1e-10): a tile pair is skipped only when its bound exceeds this
    double rmax2_up;                // > rmax^2: r < rmax implies r^2 < rmax2_up (the per-pair prefilter)
};

// Lower bound of |d - m L| over d in [lo, hi] and the integers m, for |d| < 2.5 L (compact positions).  It is the
// engine's axis_gap (ljmd_kernels.hip), a copy of its own here: a bound, not arithmetic whose roundings reach a result.
// Why it is safe for ANY rmax: the pair pass forms d = xj - xi and d' = d - L n with its own integer n, then r from the
// unfused squares.  Rounding is monotone, so d lies in [lo, hi] as computed here from the box corners, |d'| >= |d - n L|
// >= this bound for whatever n the pass picks (L m is exact for |m| <= 2), and r >= sqrt of rdf_tile_gap2, which adds
// the squares in the pass's order.  A pair with r < rmax therefore never sits in a tile pair whose bound exceeds rmax^2.
__host__ __device__ inline double rdf_axis_gap(double lo, double hi, double L)
{
    double g = __builtin_inf();
    for (int m = -2; m <= 2; ++m) {
        const double c = m * L;
        if (lo <= c && c <= hi) return 0.0;
        g = __builtin_fmin(g, __builtin_fmin(__builtin_fabs(lo - c), __builtin_fabs(hi - c)));
    }
    return g;
}

// squared lower bound of the minimum-image distance between a particle of box bi and one of box bj (6 doubles each);
// +inf when either tile is empty
__host__ __device__ inline double rdf_tile_gap2(const double *bi, const double *bj, double L)
{
    const double gx = rdf_axis_gap(bj[0] - bi[3], bj[3] - bi[0], L);
    const double gy = rdf_axis_gap(bj[1] - bi[4], bj[4] - bi[1], L);
    const double gz = rdf_axis_gap(bj[2] - bi[5], bj[5] - bi[2], L);
    return gx * gx + gy * gy + gz * gz;
}

// The two decisions of the walk, the same for the box test of a lane and for the evaluation after the ballot, in
// rdf_walk_tiles below (tests/rdf_host enumerates them on the host).
// column tile of row tile I at step u (I < T; u <= T / 2 unordered, u < T ordered: one wrap at most)
__host__ __device__ inline int rdf_walk_column(int I, int u, int T, bool unordered)
{
    int J = unordered ? I + u : u;
    if (J >= T) J -= T;
    return J;
}

// whether row tile I takes step u of a slice that ends at u1: the tie step u = T / 2 of an even T of the unordered walk
// belongs to the rows I < T / 2 only
__host__ __device__ inline bool rdf_walk_takes(int I, int u, int u1, int T, bool unordered)
{
    const int half = (unordered && (T & 1) == 0) ? T / 2 : -1;
    return u < u1 && !(u == half && I >= half);
}

// The one copy of the tile walk of rdf_pairs_kernel, stress_pairs_kernel and heatflux_pairs_kernel: the steps [u0, u1) of
// row tile I, 64 to a ballot.  Lane = step ub + lane: its column tile, whether the walk takes it from this row
// (`considered` counts these), whether the boxes keep it -- with `skip` a tile pair other than the own is left out when
// rdf_tile_gap2 exceeds bound2 (`visited` counts what is kept).  body(Jb) then runs for every kept step in ascending
// order, the column tile Jb wave-uniform.  The whole wave calls it.
template <class Body>
__device__ __forceinline__ void rdf_walk_tiles(int I, int u0, int u1, int T, bool unordered, const double *bbox, int skip, double L,
                                               double bound2, unsigned &visited, unsigned &considered, Body &&body)
{
    const int lane = threadIdx.x & 63;
    const double *bi = bbox + (size_t)I * kRdfBoxStride;
    for (int ub = u0; ub < u1; ub += 64) {
        const int u = ub + lane;
        const int J = rdf_walk_column(I, u, T, unordered);
        const bool valid = rdf_walk_takes(I, u, u1, T, unordered);
        bool keep = valid;
        if (valid && skip && J != I) keep = !(rdf_tile_gap2(bi, bbox + (size_t)J * kRdfBoxStride, L) > bound2);
        uint64_t m = __ballot(keep);
        considered += (unsigned)__popcll(__ballot(valid));
        visited += (unsigned)__popcll(m);
        while (m) {
            const int b = __builtin_ctzll(m);
            m &= m - 1;
            body(__builtin_amdgcn_readfirstlane(rdf_walk_column(I, ub + b, T, unordered)));
        }
    }
}

hipError_t launch_rdf_boxes(const RdfBoxArgs &a, hipStream_t s);
hipError_t launch_rdf_pairs(const RdfPairArgs &a, dim3 grid, hipStream_t s);

}  // namespace ljmdr
#endif
