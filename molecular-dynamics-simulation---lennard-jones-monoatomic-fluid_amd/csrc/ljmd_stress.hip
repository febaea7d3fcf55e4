// ljmd_stress.hip -- gfx950 kernels of the engine's resident pressure tensor (include/ljmd.h: ljmd_stress_*): the six
// sums of f_a d_b over the pairs within the cutoff and of v_a v_b over the particles, where the state lives, in the
// engine's tile order.
//
// Per pair pair_fixed's arithmetic (ljmd_internal.h), unfused and left to right (-ffp-contract=off, csrc/Makefile) -- the
// one copy of it is ljmd_stress_arith.h, shared with the batch engine's kernel:
//   d0 = x_i - x_j ; d = d0 - L * round(d0 * invL)              (half away from zero)
//   r2 = dx*dx + dy*dy + dz*dz ; if r2 < rc2:
//   u = 1.0 / r2 ; u3 = u*u*u ; u6 = u3*u3 ; mdu = 2.0*u6 - u3 ; fx = mdu*dx*u (fy, fz likewise)
//   terms fx*dx, fy*dy, fz*dz, fx*dy, fx*dz, fy*dz, each entering an exact integer sum as Q(t) = RNE(t 2^64).
// Under i <-> j every d and f changes sign exactly, so a term is the same from both sides: the one-rank walk evaluates an
// unordered pair once and doubles the sums.  Integer sums depend on no order: not on the slot order, the tile walk, the
// slices of the grid or the number of ranks.
//
// stress_pairs_kernel   rdf_pairs_kernel's walk (ljmd_rdf.h: RdfPairArgs, rdf_walk_tiles): one wave per row tile, lane =
//                       own particle in registers, column coordinates wave-uniform; 64 column tiles are tested at a
//                       time, lane = column tile, with rdf_tile_gap2.  Six 128-bit accumulators per lane (fewer than
//                       2^23 terms below 2^104 each); after the walk integer shuffles across the wave, the workgroup's
//                       waves through LDS, and ONE 192-bit partial per component, the range flag (workgroup_sum192,
//                       ljmd_sum192.h) and the two tile-pair counts go to the workgroup's own rows by plain stores.
// stress_kinetic_kernel the six velocity products of kStressKinBlock slots per workgroup, reduced the same way
//                       (series_kinetic, ljmd_sum192.h).
// series_fold_kernel<6, 6> (ljmd_sum192.h)  one workgroup, one wave per output row: adds the partials in 192 bits, writes
//                       row s of the series (its only writer), the tile-pair counts of this accumulate, and ORs the
//                       flags into the sticky word.
// No global atomics, no floating-point atomics, no spin-waits, no dependency between workgroups inside a launch.
#include "ljmd_stress.h"

#include "ljmd_internal.h"
#include "ljmd_stress_arith.h"
#include "ljmd_sum192.h"

namespace ljmds {
namespace {

static_assert(kStressComponents == ljmdk::kStressTerms, "the shared arithmetic adds six terms");

static_assert(kStressFoldWaves == 2 * kStressComponents + 1, "one wave per row of the fold");

using ljmdk::add_six;
using ljmdk::kTile;
using ljmdk::series_kinetic;
using ljmdk::series_kinetic_ok;
using ljmdk::stress_image;
using ljmdk::stress_terms;
using ljmdk::workgroup_sum192;
using ljmdr::rdf_walk_tiles;

// the 64 x 64 pairs of one (row tile, column tile).  MODE 0: all of them; 1: column slot > row slot (the diagonal tile of
// the unordered walk); 2: column slot != row slot (the own tile of the ordered walk)
template <int MODE>
__device__ __forceinline__ void tile_pairs(const StressPairArgs &a, const double *bx, double xi, double yi, double zi,
                                           int lane, __int128 (&acc)[kStressComponents], bool &bad)
{
    const double *by = bx + a.P, *bz = by + a.P;
    for (int j0 = 0; j0 < kTile; j0 += 8) {
        double xj[8], yj[8], zj[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) { xj[k] = bx[j0 + k]; yj[k] = by[j0 + k]; zj[k] = bz[j0 + k]; }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const double dx0 = xi - xj[k], dy0 = yi - yj[k], dz0 = zi - zj[k];
            const double dx = stress_image(dx0, a.L, a.invL);
            const double dy = stress_image(dy0, a.L, a.invL);
            const double dz = stress_image(dz0, a.L, a.invL);
            const double r2 = dx * dx + dy * dy + dz * dz;
            bool in = r2 < a.rc2;                                   // NaN (padding) never passes
            if (MODE == 1) in = in && (j0 + k > lane);
            if (MODE == 2) in = in && (j0 + k != lane);
            if (in) {
                double t[kStressComponents];
                const bool oob = stress_terms(dx, dy, dz, r2, t);
                add_six(acc, t, oob, bad);
            }
        }
    }
}

__global__ __launch_bounds__(kRdfWaves * kTile) void stress_pairs_kernel(StressPairArgs a)
{
    __shared__ uint64_t wsum[kRdfWaves][kStressComponents][3];
    __shared__ unsigned wcount[kRdfWaves][2];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int Il = blockIdx.x * kRdfWaves + wave;               // own row tile, wave-uniform
    const bool unordered = a.G == 1;
    __int128 acc[kStressComponents] = {0, 0, 0, 0, 0, 0};
    bool bad = false;
    unsigned visited = 0, considered = 0;
    if (Il < a.TB) {
        const int I = a.rank * a.TB + Il;
        const int row = Il * kTile + lane;
        const double *own = a.pos + (size_t)a.rank * 3 * a.P;
        const double xi = own[row], yi = own[a.P + row], zi = own[2 * (size_t)a.P + row];
        const int u0 = blockIdx.y * a.chunk, u1 = min(u0 + a.chunk, a.U);
        rdf_walk_tiles(I, u0, u1, a.T, unordered, a.bbox, a.skip, a.L, a.rc2_skin, visited, considered, [&](int Jb) {
            const int gj = unordered ? 0 : Jb / a.TB;
            const double *bx = a.pos + (size_t)gj * 3 * a.P + (size_t)(Jb - gj * a.TB) * kTile;
            if (Jb != I)
                tile_pairs<0>(a, bx, xi, yi, zi, lane, acc, bad);
            else if (unordered)
                tile_pairs<1>(a, bx, xi, yi, zi, lane, acc, bad);
            else
                tile_pairs<2>(a, bx, xi, yi, zi, lane, acc, bad);
        });
    }
    if (lane == 0) {
        wcount[wave][0] = visited;
        wcount[wave][1] = considered;
    }

    // the workgroup's own rows: threads 0..5 the sums (both orders of every pair of the unordered walk), thread 6 the
    // flag, threads 7 and 8 the two counts -- wcount is complete behind the barrier of workgroup_sum192
    const size_t wg = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    workgroup_sum192(acc, unordered, bad, lane, wave, wsum, a.part, a.pflag, wg);
    if (threadIdx.x > kStressComponents && threadIdx.x <= kStressComponents + 2) {
        const int k = threadIdx.x - kStressComponents - 1;
        unsigned long long n = 0;
        for (int w = 0; w < kRdfWaves; ++w) n += wcount[w][k];
        a.pcount[wg * 2 + k] = n;
    }
}

__global__ __launch_bounds__(kStressKinThreads) void stress_kinetic_kernel(StressKineticArgs a)
{
    series_kinetic<kStressComponents, kStressKinThreads, kStressKinPerThread>(
        a, [](__int128(&acc)[kStressComponents], double vx, double vy, double vz, bool &bad) {
            const double t[kStressComponents] = {vx * vx, vy * vy, vz * vz, vx * vy, vx * vz, vy * vz};
            add_six(acc, t, false, bad);
        });
}

}  // namespace

hipError_t launch_stress_pairs(const StressPairArgs &a, dim3 grid, hipStream_t s)
{
    // what the kernel's indexing and its 128-bit lane accumulators rest on
    if (!a.pos || !a.bbox || !a.part || !a.pcount || !a.pflag || a.chunk < 1 || a.U < 1 || a.TB < 1 || a.P < a.TB * kTile ||
        a.T != a.G * a.TB || a.rank < 0 || a.rank >= a.G || (a.G == 1 ? a.U != a.T / 2 + 1 : a.U != a.T) ||
        (long long)a.T * kTile > (long long)kStressMaxN + 256 * (long long)a.G ||
        (long long)grid.x * kRdfWaves < a.TB || (long long)grid.y * a.chunk < a.U || grid.z != 1)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(stress_pairs_kernel, grid, dim3(kRdfWaves * kTile), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_stress_kinetic(const StressKineticArgs &a, hipStream_t s)
{
    if (!series_kinetic_ok(a, kStressKinBlock)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(stress_kinetic_kernel, dim3(a.blocks), dim3(kStressKinThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_stress_fold(const StressFoldArgs &a, hipStream_t s)
{
    return ljmdk::launch_series_fold<kStressComponents, kStressComponents>(a, s);      // K[6][3], then S[6][3]
}

}  // namespace ljmds
