// ljmd_current.hip -- gfx950 kernels of the engine's resident current modes (include/ljmd.h: ljmd_current_*): the sums
// of Q(v_a cos k . r_j) and Q(v_a sin k . r_j), a = x, y, z, over the live particles for every mode of the configured
// list, where the state lives, in the engine's slot order.  One-rank engines only.  The arithmetic of a term is
// ljmd_current_arith.h over ljmd_rhok_arith.h, unfused (-ffp-contract=off, csrc/Makefile); every term enters an exact
// integer sum as Q(t) = RNE(t 2^64), so the words depend on no order: not on the slot order, the re-sorts or the grid.
//
// current_terms_kernel  lanes <-> modes, as rhok_terms_kernel.  A wave is a unit of its own: 64 modes, one per lane with
//                       its integer triple in registers, and a chunk of `tiles` 64-slot tiles.  Per tile lane l loads
//                       slot l: its id, its coordinates reduced to turns and its three velocities; the wave then walks
//                       the live slots of the tile -- the ballot of the ids in [0, n); a padding slot adds nothing and
//                       sets no flag -- taking the slot's six values wave-uniform from lane j (v_readlane: no LDS, no
//                       barrier).  Every lane adds the six Q of its own mode, each into a signed 128-bit sum, so no
//                       cross-lane reduction is needed.  The unit's row of partials [mode][a][Re, Im][3] and its range
//                       flag go out by plain stores.
// current_fold_kernel   one workgroup per mode chunk, lane = mode, wave w adds the rows w, w + 4, ... of the particle
//                       chunks in 192 bits; the waves meet in LDS (kCurrentFoldWaves, ljmd_current.h), wave 0 writes the
//                       mode's eighteen words of row `snapshot` of the series (its only writer) and ORs the flags into
//                       the sticky word.
// No global atomics, no floating-point atomics, no spin-waits, no dependency between workgroups inside a launch.
#include "ljmd_current.h"

#include "ljmd_current_arith.h"
#include "ljmd_internal.h"

namespace ljmdc {
namespace {

using ljmdk::add192;
using ljmdk::from128;
using ljmdk::kTile;

static_assert(kTile == kRhokModeChunk, "lane l stages slot l of a tile and owns mode l of a chunk");
static_assert(ljmdk::kCurrentBound == ljmdk::kFixedBound, "the range rule is that of the reproducible mode");
// A term has |Q| < 2^104 (|t| < kFixedBound = 2^40).  A lane adds one term per live slot of its chunk, at most
// n <= kFixedMaxN = 2^23 of them, so every one of its six sums stays below 2^23 2^104 = 2^127: it fits a signed 128-bit
// integer, with no carry to watch.
static_assert(kRhokMaxN == ljmdk::kFixedMaxN && ljmdk::kFixedMaxN <= (1 << 23), "the lane accumulators rest on kFixedMaxN");

// lane `j` (wave-uniform) of x, in SGPRs
__device__ __forceinline__ double lane_value(double x, int j)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(x), j);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(x), j);
    return __hiloint2double(hi, lo);
}

__global__ __launch_bounds__(kCurrentWaves * 64) void current_terms_kernel(CurrentTermsArgs a)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int unit = blockIdx.x * kCurrentWaves + wave;        // wave-uniform
    if (unit >= a.pchunks * a.mchunks) return;
    const int y = unit % a.mchunks, p = unit / a.mchunks;
    const int m = y * kRhokModeChunk + lane;
    const bool mode_live = m < a.n_modes;
    // a lane without a mode runs mode (0, 0, 0) and stores zeros into the padding of its row
    const double nx = mode_live ? (double)a.modes[3 * m] : 0.0;
    const double ny = mode_live ? (double)a.modes[3 * m + 1] : 0.0;
    const double nz = mode_live ? (double)a.modes[3 * m + 2] : 0.0;

    __int128 acc[kCurrentSums] = {0, 0, 0, 0, 0, 0};
    bool bad = false;
    const size_t P = (size_t)a.P;
    const int t0 = p * a.tiles, t1 = min(t0 + a.tiles, a.T);
    for (int t = t0; t < t1; ++t) {
        const size_t s = (size_t)t * kTile + lane;              // < T 64 <= P
        const int id = a.perm[s];
        const double tx = ljmdk::rhok_turns(a.pos[s], a.L);
        const double ty = ljmdk::rhok_turns(a.pos[P + s], a.L);
        const double tz = ljmdk::rhok_turns(a.pos[2 * P + s], a.L);
        const double vx = a.v[s], vy = a.v[P + s], vz = a.v[2 * P + s];
        unsigned long long live = __ballot(id >= 0 && id < a.n);
        while (live) {
            const int j = __builtin_ctzll(live);
            live &= live - 1;
            const double ux = lane_value(tx, j), uy = lane_value(ty, j), uz = lane_value(tz, j);
            const double wx = lane_value(vx, j), wy = lane_value(vy, j), wz = lane_value(vz, j);
            double C, S, term[kCurrentSums];
            ljmdk::rhok_term(nx, ny, nz, ux, uy, uz, C, S);
            ljmdk::current_products(wx, wy, wz, C, S, term);
            const bool oob = ljmdk::current_out_of_range(C, S, term);
            bad = bad || oob;
#pragma unroll
            for (int k = 0; k < kCurrentSums; ++k) ljmdk::current_fixed_add(acc[k], oob ? 0.0 : term[k]);
        }
    }
    uint64_t *row = a.part + ((size_t)p * a.mchunks * kRhokModeChunk + m) * kCurrentRowWords;
#pragma unroll
    for (int k = 0; k < kCurrentSums; ++k) {
        uint64_t q[3];
        from128(q, acc[k]);
        row[3 * k] = mode_live ? q[0] : 0; row[3 * k + 1] = mode_live ? q[1] : 0; row[3 * k + 2] = mode_live ? q[2] : 0;
    }
    const bool any_bad = __any(bad && mode_live);
    if (lane == 0) a.flag[(size_t)p * a.mchunks + y] = any_bad ? 1u : 0u;
}

__global__ __launch_bounds__(kCurrentFoldWaves * 64) void current_fold_kernel(CurrentFoldArgs a)
{
    __shared__ uint64_t wsum[kCurrentFoldWaves][kCurrentRowWords][64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int y = blockIdx.x;
    const int m = y * kRhokModeChunk + lane;
    uint64_t sum[kCurrentSums][3] = {};
    unsigned bad = 0;
    for (int p = wave; p < a.pchunks; p += kCurrentFoldWaves) {
        const uint64_t *src = a.part + ((size_t)p * a.mchunks * kRhokModeChunk + m) * kCurrentRowWords;
#pragma unroll
        for (int k = 0; k < kCurrentSums; ++k) {
            const uint64_t o[3] = {src[3 * k], src[3 * k + 1], src[3 * k + 2]};
            add192(sum[k], o);
        }
        bad |= a.flag[(size_t)p * a.mchunks + y];
    }
#pragma unroll
    for (int k = 0; k < kCurrentSums; ++k)
#pragma unroll
        for (int w = 0; w < 3; ++w) wsum[wave][3 * k + w][lane] = sum[k][w];
    const int any_bad = __syncthreads_or(bad != 0 ? 1 : 0);
    if (wave != 0) return;
    for (int o = 1; o < kCurrentFoldWaves; ++o) {
#pragma unroll
        for (int k = 0; k < kCurrentSums; ++k) {
            const uint64_t q[3] = {wsum[o][3 * k][lane], wsum[o][3 * k + 1][lane], wsum[o][3 * k + 2][lane]};
            add192(sum[k], q);
        }
    }
    if (m < a.n_modes) {
        uint64_t *dst = a.row + (size_t)m * kCurrentRowWords;
#pragma unroll
        for (int k = 0; k < kCurrentSums; ++k)
#pragma unroll
            for (int w = 0; w < 3; ++w) dst[3 * k + w] = sum[k][w];
    }
    if (any_bad && lane == 0) *a.range = 1;                     // every writer stores the same value
}

}  // namespace

hipError_t launch_current_terms(const CurrentTermsArgs &a, hipStream_t s)
{
    if (!current_terms_ok(a)) return hipErrorInvalidValue;
    const int units = a.pchunks * a.mchunks;
    hipLaunchKernelGGL(current_terms_kernel, dim3((units + kCurrentWaves - 1) / kCurrentWaves), dim3(kCurrentWaves * 64), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_current_fold(const CurrentFoldArgs &a, hipStream_t s)
{
    if (!current_fold_ok(a)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(current_fold_kernel, dim3(a.mchunks), dim3(kCurrentFoldWaves * 64), 0, s, a);
    return hipGetLastError();
}

}  // namespace ljmdc
