// ljmd_stress.hip -- gfx950 kernels of the engine's resident pressure tensor (include/ljmd.h: ljmd_stress_*): the six
// sums of f_a d_b over the pairs within the cutoff and of v_a v_b over the particles, where the state lives, in the
// engine's tile order.
//
// Per pair pair_fixed's arithmetic (ljmd_internal.h), unfused and left to right (-ffp-contract=off, csrc/Makefile) -- the
// one copy of it, with add_six and wave_sum192, is ljmd_stress_arith.h, shared with the batch engine's kernel:
//   d0 = x_i - x_j ; d = d0 - L * round(d0 * invL)              (half away from zero)
//   r2 = dx*dx + dy*dy + dz*dz ; if r2 < rc2:
//   u = 1.0 / r2 ; u3 = u*u*u ; u6 = u3*u3 ; mdu = 2.0*u6 - u3 ; fx = mdu*dx*u (fy, fz likewise)
//   terms fx*dx, fy*dy, fz*dz, fx*dy, fx*dz, fy*dz, each entering an exact integer sum as Q(t) = RNE(t 2^64).
// Under i <-> j every d and f changes sign exactly, so a term is the same from both sides: the one-rank walk evaluates an
// unordered pair once and doubles the sums.  Integer sums depend on no order: not on the slot order, the tile walk, the
// slices of the grid or the number of ranks.
//
// stress_pairs_kernel   rdf_pairs_kernel's walk (ljmd_rdf.h: RdfPairArgs): one wave per row tile, lane = own particle in
//                       registers, column coordinates wave-uniform; 64 column tiles are tested at a time, lane = column
//                       tile, with rdf_tile_gap2.  Six 128-bit accumulators per lane (fewer than 2^23 terms below 2^104
//                       each); after the walk integer shuffles across the wave, the workgroup's waves through LDS, and
//                       ONE 192-bit partial per component, the range flag and the two tile-pair counts go to the
//                       workgroup's own rows by plain stores.
// stress_kinetic_kernel the six velocity products of kStressKinBlock slots per workgroup, reduced the same way.
// stress_fold_kernel    one workgroup, one wave per output row: adds the partials in 192 bits, writes row s of the series
//                       (its only writer), the tile-pair counts of this accumulate, and ORs the flags into the sticky word.
// No global atomics, no floating-point atomics, no spin-waits, no dependency between workgroups inside a launch.
#include "ljmd_stress.h"

#include "ljmd_internal.h"
#include "ljmd_stress_arith.h"

namespace ljmds {
namespace {

static_assert(kStressComponents == ljmdk::kStressTerms, "the shared arithmetic adds six terms");

using ljmdk::add192;
using ljmdk::add_six;
using ljmdk::from128;
using ljmdk::kTile;
using ljmdk::stress_image;
using ljmdk::stress_terms;
using ljmdk::wave_sum192;
using ljmdr::rdf_tile_gap2;
using ljmdr::rdf_walk_column;
using ljmdr::rdf_walk_takes;

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
        const double *bi = a.bbox + (size_t)I * kRdfBoxStride;
        const int u0 = blockIdx.y * a.chunk, u1 = min(u0 + a.chunk, a.U);
        for (int ub = u0; ub < u1; ub += 64) {
            // lane = step ub + lane: its column tile, whether the walk takes it from this row, whether the boxes keep it
            const int u = ub + lane;
            const int J = rdf_walk_column(I, u, a.T, unordered);
            const bool valid = rdf_walk_takes(I, u, u1, a.T, unordered);
            bool keep = valid;
            if (valid && a.skip && J != I) keep = !(rdf_tile_gap2(bi, a.bbox + (size_t)J * kRdfBoxStride, a.L) > a.rc2_skin);
            uint64_t m = __ballot(keep);
            considered += (unsigned)__popcll(__ballot(valid));
            visited += (unsigned)__popcll(m);
            while (m) {
                const int b = __builtin_ctzll(m);
                m &= m - 1;
                const int Jb = __builtin_amdgcn_readfirstlane(rdf_walk_column(I, ub + b, a.T, unordered));
                const int gj = unordered ? 0 : Jb / a.TB;
                const double *bx = a.pos + (size_t)gj * 3 * a.P + (size_t)(Jb - gj * a.TB) * kTile;
                if (Jb != I)
                    tile_pairs<0>(a, bx, xi, yi, zi, lane, acc, bad);
                else if (unordered)
                    tile_pairs<1>(a, bx, xi, yi, zi, lane, acc, bad);
                else
                    tile_pairs<2>(a, bx, xi, yi, zi, lane, acc, bad);
            }
        }
    }

    // lanes -> wave: 192 bits from here on (64 lanes of 2^127, doubled, do not fit 128)
#pragma unroll
    for (int c = 0; c < kStressComponents; ++c) {
        uint64_t q[3];
        from128(q, acc[c]);
        if (unordered) {                                        // both orders of every pair
            const uint64_t o[3] = {q[0], q[1], q[2]};
            add192(q, o);
        }
        wave_sum192(q);
        if (lane == 0) {
            wsum[wave][c][0] = q[0];
            wsum[wave][c][1] = q[1];
            wsum[wave][c][2] = q[2];
        }
    }
    if (lane == 0) {
        wcount[wave][0] = visited;
        wcount[wave][1] = considered;
    }
    const int any_bad = __syncthreads_or(bad ? 1 : 0);          // the one barrier: wsum and wcount are complete behind it

    // waves -> workgroup: thread c adds component c, thread 6 + k count k, into the workgroup's own rows
    const size_t wg = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    if (threadIdx.x < kStressComponents) {
        const int c = threadIdx.x;
        uint64_t q[3] = {wsum[0][c][0], wsum[0][c][1], wsum[0][c][2]};
        for (int w = 1; w < kRdfWaves; ++w) {
            const uint64_t o[3] = {wsum[w][c][0], wsum[w][c][1], wsum[w][c][2]};
            add192(q, o);
        }
        uint64_t *dst = a.part + (wg * kStressComponents + c) * 3;
        dst[0] = q[0];
        dst[1] = q[1];
        dst[2] = q[2];
    } else if (threadIdx.x < kStressComponents + 2) {
        const int k = threadIdx.x - kStressComponents;
        unsigned long long n = 0;
        for (int w = 0; w < kRdfWaves; ++w) n += wcount[w][k];
        a.pcount[wg * 2 + k] = n;
    } else if (threadIdx.x == kStressComponents + 2) {
        a.pflag[wg] = any_bad ? 1u : 0u;
    }
}

__global__ __launch_bounds__(kStressKinThreads) void stress_kinetic_kernel(StressKineticArgs a)
{
    constexpr int kWaves = kStressKinThreads / 64;
    __shared__ uint64_t wsum[kWaves][kStressComponents][3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __int128 acc[kStressComponents] = {0, 0, 0, 0, 0, 0};
    bool bad = false;
    const size_t P = (size_t)a.P;
    const size_t s0 = (size_t)blockIdx.x * kStressKinBlock + threadIdx.x;
#pragma unroll 1
    for (int k = 0; k < kStressKinPerThread; ++k) {
        const size_t s = s0 + (size_t)k * kStressKinThreads;
        if (s >= P) break;
        const double vx = a.v[s], vy = a.v[P + s], vz = a.v[2 * P + s];      // a padding slot holds 0: Q(0) = 0
        const double t[kStressComponents] = {vx * vx, vy * vy, vz * vz, vx * vy, vx * vz, vy * vz};
        add_six(acc, t, false, bad);
    }
#pragma unroll
    for (int c = 0; c < kStressComponents; ++c) {
        uint64_t q[3];
        from128(q, acc[c]);
        wave_sum192(q);
        if (lane == 0) {
            wsum[wave][c][0] = q[0];
            wsum[wave][c][1] = q[1];
            wsum[wave][c][2] = q[2];
        }
    }
    const int any_bad = __syncthreads_or(bad ? 1 : 0);
    if (threadIdx.x < kStressComponents) {
        const int c = threadIdx.x;
        uint64_t q[3] = {wsum[0][c][0], wsum[0][c][1], wsum[0][c][2]};
        for (int w = 1; w < kWaves; ++w) {
            const uint64_t o[3] = {wsum[w][c][0], wsum[w][c][1], wsum[w][c][2]};
            add192(q, o);
        }
        uint64_t *dst = a.kpart + ((size_t)blockIdx.x * kStressComponents + c) * 3;
        dst[0] = q[0];
        dst[1] = q[1];
        dst[2] = q[2];
    } else if (threadIdx.x == kStressComponents) {
        a.kflag[blockIdx.x] = any_bad ? 1u : 0u;
    }
}

__global__ __launch_bounds__(kStressFoldWaves * 64) void stress_fold_kernel(StressFoldArgs a)
{
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);      // output row of this wave
    if (w < 2 * kStressComponents) {
        const bool kin = w < kStressComponents;
        const int c = kin ? w : w - kStressComponents;
        const uint64_t *src = kin ? a.kpart : a.part;
        const unsigned *flg = kin ? a.kflag : a.pflag;
        const int rows = kin ? a.blocks : a.workgroups;
        uint64_t q[3] = {0, 0, 0};
        unsigned bad = 0;
        for (int r = lane; r < rows; r += 64) {
            const uint64_t *p = src + ((size_t)r * kStressComponents + c) * 3;
            const uint64_t o[3] = {p[0], p[1], p[2]};
            add192(q, o);
            bad |= flg[r];
        }
        wave_sum192(q);
        const bool any_bad = __any(bad != 0);
        if (lane == 0) {
            uint64_t *dst = a.row + (size_t)w * 3;              // K[6][3], then S[6][3]
            dst[0] = q[0];
            dst[1] = q[1];
            dst[2] = q[2];
            if (any_bad && c == 0) *a.range = 1;                // every writer stores the same value
        }
    } else {
        unsigned long long n0 = 0, n1 = 0;
        for (int r = lane; r < a.workgroups; r += 64) {
            n0 += a.pcount[2 * (size_t)r];
            n1 += a.pcount[2 * (size_t)r + 1];
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            n0 += __shfl_down(n0, off, 64);
            n1 += __shfl_down(n1, off, 64);
        }
        if (lane == 0) {
            a.count[0] = n0;
            a.count[1] = n1;
        }
    }
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
    if (!a.v || !a.kpart || !a.kflag || a.P < 1 || a.blocks < 1 || (long long)a.blocks * kStressKinBlock < a.P ||
        (long long)(a.blocks - 1) * kStressKinBlock >= a.P)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(stress_kinetic_kernel, dim3(a.blocks), dim3(kStressKinThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_stress_fold(const StressFoldArgs &a, hipStream_t s)
{
    if (!a.part || !a.pcount || !a.pflag || !a.kpart || !a.kflag || !a.row || !a.count || !a.range || a.workgroups < 1 ||
        a.blocks < 1)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(stress_fold_kernel, dim3(1), dim3(kStressFoldWaves * 64), 0, s, a);
    return hipGetLastError();
}

}  // namespace ljmds
