// ljmd_heatflux.hip -- gfx950 kernels of the engine's resident heat flux (include/ljmd.h: ljmd_heatflux_*): the sums of
// phi (v_i + v_j) and of (f . (v_i + v_j)) d over the pairs within the cutoff and of v^2 v over the particles, where the
// state lives, in the engine's tile order.  One-rank engines only: a pair needs the column particle's velocity.
//
// Per pair the pressure tensor's arithmetic (ljmd_stress_arith.h), unfused and left to right (-ffp-contract=off,
// csrc/Makefile), and on top of it (ljmd_heatflux_arith.h):
//   d0 = x_i - x_j ; d = d0 - L * round(d0 * invL)              (half away from zero)
//   r2 = dx*dx + dy*dy + dz*dz ; if r2 < rc2:
//   u = 1.0 / r2 ; u3 = u*u*u ; u6 = u3*u3 ; mdu = 2.0*u6 - u3 ; fx = mdu*dx*u (fy, fz likewise)
//   wx = vx_i + vx_j (wy, wz likewise) ; phi = u6 - u3 ; g = fx*wx + fy*wy + fz*wz
//   terms phi*wx, phi*wy, phi*wz, g*dx, g*dy, g*dz, each entering an exact integer sum as Q(t) = RNE(t 2^64).
// Under i <-> j w, r2 and phi keep their bits, every d, f and g change sign exactly, so a term is the same from both
// sides: the walk evaluates an unordered pair once and doubles the sums.  Integer sums depend on no order: not on the
// slot order, the tile walk or the slices of the grid.
//
// heatflux_pairs_kernel   stress_pairs_kernel's unordered walk (ljmd_rdf.h: rdf_walk_tiles): one wave per row tile, lane = own particle
//                         with its position and velocity in registers, column positions and velocities wave-uniform,
//                         kHeatfluxColumns at a time; 64 column tiles are tested at a time, lane = column tile, with
//                         rdf_tile_gap2.  Six 128-bit accumulators per lane (fewer than 2^23 terms below 2^104 each);
//                         after the walk integer shuffles across the wave, the workgroup's waves through LDS, and ONE
//                         192-bit partial per component, the range flag (workgroup_sum192, ljmd_sum192.h) and the two
//                         tile-pair counts go to the workgroup's own rows by plain stores.
// heatflux_kinetic_kernel the three terms k2 v_a of kHeatfluxKinBlock slots per workgroup, reduced the same way
//                         (series_kinetic, ljmd_sum192.h).
// series_fold_kernel<3, 6> (ljmd_sum192.h)  one workgroup, one wave per output row: adds the partials in 192 bits, writes
//                         row s of the series (its only writer), the tile-pair counts of this accumulate, and ORs the
//                         flags into the sticky word.
// No global atomics, no floating-point atomics, no spin-waits, no dependency between workgroups inside a launch.
#include "ljmd_heatflux.h"

#include "ljmd_heatflux_arith.h"
#include "ljmd_internal.h"
#include "ljmd_sum192.h"

namespace ljmdq {
namespace {

static_assert(kHeatfluxPairComponents == ljmdk::kHeatfluxPairTerms && kHeatfluxKinComponents == ljmdk::kHeatfluxKinTerms,
              "the arithmetic header adds six pair terms and three particle terms");
static_assert(ljmdk::kTile % kHeatfluxColumns == 0, "a tile is a whole number of column batches");

static_assert(kHeatfluxFoldWaves == kHeatfluxKinComponents + kHeatfluxPairComponents + 1, "one wave per row of the fold");

using ljmdk::add_six;
using ljmdk::heatflux_add_kinetic;
using ljmdk::heatflux_terms;
using ljmdk::kTile;
using ljmdk::series_kinetic;
using ljmdk::series_kinetic_ok;
using ljmdk::stress_image;
using ljmdk::workgroup_sum192;
using ljmdr::rdf_walk_tiles;

// the 64 x 64 pairs of one (row tile, column tile); bx / bv: x of the column tile's first slot in pos / vel.  DIAGONAL:
// column slot > row slot only
template <bool DIAGONAL>
__device__ __forceinline__ void tile_pairs(const HeatfluxPairArgs &a, const double *bx, const double *bv, double xi, double yi,
                                           double zi, double vxi, double vyi, double vzi, int lane,
                                           __int128 (&acc)[kHeatfluxPairComponents], bool &bad)
{
    constexpr int B = kHeatfluxColumns;
    const double *by = bx + a.P, *bz = by + a.P;
    const double *bvy = bv + a.P, *bvz = bvy + a.P;
    for (int j0 = 0; j0 < kTile; j0 += B) {
        double xj[B], yj[B], zj[B], vxj[B], vyj[B], vzj[B];
#pragma unroll
        for (int k = 0; k < B; ++k) {
            xj[k] = bx[j0 + k]; yj[k] = by[j0 + k]; zj[k] = bz[j0 + k];
            vxj[k] = bv[j0 + k]; vyj[k] = bvy[j0 + k]; vzj[k] = bvz[j0 + k];
        }
#pragma unroll
        for (int k = 0; k < B; ++k) {
            const double dx0 = xi - xj[k], dy0 = yi - yj[k], dz0 = zi - zj[k];
            const double dx = stress_image(dx0, a.L, a.invL);
            const double dy = stress_image(dy0, a.L, a.invL);
            const double dz = stress_image(dz0, a.L, a.invL);
            const double r2 = dx * dx + dy * dy + dz * dz;
            bool in = r2 < a.rc2;                                   // NaN (padding) never passes
            if (DIAGONAL) in = in && (j0 + k > lane);
            if (in) {
                double t[kHeatfluxPairComponents];
                const bool oob = heatflux_terms(dx, dy, dz, r2, vxi + vxj[k], vyi + vyj[k], vzi + vzj[k], t);
                add_six(acc, t, oob, bad);
            }
        }
    }
}

__global__ __launch_bounds__(kRdfWaves * kTile) void heatflux_pairs_kernel(HeatfluxPairArgs a)
{
    __shared__ uint64_t wsum[kRdfWaves][kHeatfluxPairComponents][3];
    __shared__ unsigned wcount[kRdfWaves][2];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int I = blockIdx.x * kRdfWaves + wave;                // own row tile, wave-uniform
    __int128 acc[kHeatfluxPairComponents] = {0, 0, 0, 0, 0, 0};
    bool bad = false;
    unsigned visited = 0, considered = 0;
    if (I < a.T) {
        const size_t row = (size_t)I * kTile + lane, P = (size_t)a.P;
        const double xi = a.pos[row], yi = a.pos[P + row], zi = a.pos[2 * P + row];
        const double vxi = a.vel[row], vyi = a.vel[P + row], vzi = a.vel[2 * P + row];
        const int u0 = blockIdx.y * a.chunk, u1 = min(u0 + a.chunk, a.U);
        rdf_walk_tiles(I, u0, u1, a.T, true, a.bbox, a.skip, a.L, a.rc2_skin, visited, considered, [&](int Jb) {
            const double *bx = a.pos + (size_t)Jb * kTile, *bv = a.vel + (size_t)Jb * kTile;
            if (Jb != I)
                tile_pairs<false>(a, bx, bv, xi, yi, zi, vxi, vyi, vzi, lane, acc, bad);
            else
                tile_pairs<true>(a, bx, bv, xi, yi, zi, vxi, vyi, vzi, lane, acc, bad);
        });
    }
    if (lane == 0) {
        wcount[wave][0] = visited;
        wcount[wave][1] = considered;
    }

    // the workgroup's own rows: threads 0..5 the sums (both orders of every pair), thread 6 the flag, threads 7 and 8
    // the two counts -- wcount is complete behind the barrier of workgroup_sum192
    const size_t wg = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    workgroup_sum192(acc, true, bad, lane, wave, wsum, a.part, a.pflag, wg);
    if (threadIdx.x > kHeatfluxPairComponents && threadIdx.x <= kHeatfluxPairComponents + 2) {
        const int k = threadIdx.x - kHeatfluxPairComponents - 1;
        unsigned long long n = 0;
        for (int w = 0; w < kRdfWaves; ++w) n += wcount[w][k];
        a.pcount[wg * 2 + k] = n;
    }
}

__global__ __launch_bounds__(kHeatfluxKinThreads) void heatflux_kinetic_kernel(HeatfluxKineticArgs a)
{
    series_kinetic<kHeatfluxKinComponents, kHeatfluxKinThreads, kHeatfluxKinPerThread>(
        a, [](__int128(&acc)[kHeatfluxKinComponents], double vx, double vy, double vz, bool &bad) {
            heatflux_add_kinetic(acc, vx, vy, vz, bad);
        });
}

}  // namespace

hipError_t launch_heatflux_pairs(const HeatfluxPairArgs &a, dim3 grid, hipStream_t s)
{
    // what the kernel's indexing and its 128-bit lane accumulators rest on
    if (!a.pos || !a.vel || !a.bbox || !a.part || !a.pcount || !a.pflag || a.chunk < 1 || a.U < 1 || a.T < 1 ||
        (long long)a.P < (long long)a.T * kTile || a.U != a.T / 2 + 1 || (long long)a.T * kTile > (long long)kHeatfluxMaxN + 256 ||
        (long long)grid.x * kRdfWaves < a.T || (long long)grid.y * a.chunk < a.U || grid.z != 1)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(heatflux_pairs_kernel, grid, dim3(kRdfWaves * kTile), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_heatflux_kinetic(const HeatfluxKineticArgs &a, hipStream_t s)
{
    if (!series_kinetic_ok(a, kHeatfluxKinBlock)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(heatflux_kinetic_kernel, dim3(a.blocks), dim3(kHeatfluxKinThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_heatflux_fold(const HeatfluxFoldArgs &a, hipStream_t s)
{
    return ljmdk::launch_series_fold<kHeatfluxKinComponents, kHeatfluxPairComponents>(a, s);   // E[3][3], then P[3][3], C[3][3]
}

}  // namespace ljmdq
