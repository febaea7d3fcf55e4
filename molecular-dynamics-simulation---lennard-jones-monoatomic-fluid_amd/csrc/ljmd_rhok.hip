// ljmd_rhok.hip -- gfx950 kernels of the engine's resident density modes (include/ljmd.h: ljmd_rhok_*): the sums of
// Q(cos k . r_j) and Q(sin k . r_j) over the live particles for every mode of the configured list, where the state
// lives, in the engine's slot order.  One-rank engines only.  The arithmetic of a term is ljmd_rhok_arith.h, unfused
// (-ffp-contract=off, csrc/Makefile); every term enters an exact integer sum as Q(t) = RNE(t 2^64), so the words depend
// on no order: not on the slot order, the re-sorts or the grid.
//
// rhok_terms_kernel   lanes <-> modes.  A wave is a unit of its own: 64 modes, one per lane with its integer triple in
//                     registers, and a chunk of `tiles` 64-slot tiles.  Per tile lane l loads slot l, its id and reduces
//                     its coordinates to turns (one division per coordinate and slot, not one per mode); the wave then
//                     walks the live slots of the tile -- the ballot of the ids in [0, n); a padding slot adds nothing and
//                     sets no flag -- taking the slot's three turns wave-uniform from lane j (v_readlane: no LDS, no
//                     barrier).  Every lane adds Q(C) and Q(S) of its own mode, each as two 64-bit parts (ljmd_rhok_arith.h),
//                     so no cross-lane reduction is needed.  The unit's row of partials [mode][Re[3], Im[3]] and its range
//                     flag go out by plain stores.
// rhok_fold_kernel    one workgroup per mode chunk, lane = mode, wave w adds the rows w, w + 8, ... of the particle
//                     chunks in 192 bits; the waves meet in LDS, wave 0 writes the mode's six words of row `snapshot` of
//                     the series (its only writer) and ORs the flags into the sticky word.
// No global atomics, no floating-point atomics, no spin-waits, no dependency between workgroups inside a launch.
#include "ljmd_rhok.h"

#include "ljmd_internal.h"
#include "ljmd_rhok_arith.h"

namespace ljmdc {
namespace {

using ljmdk::add192;
using ljmdk::from128;
using ljmdk::kTile;

static_assert(kTile == kRhokModeChunk, "lane l stages slot l of a tile and owns mode l of a chunk");
static_assert(kRhokMaxN == ljmdk::kFixedMaxN, "the lane accumulators rest on kFixedMaxN");

// lane `j` (wave-uniform) of x, in SGPRs
__device__ __forceinline__ double lane_value(double x, int j)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(x), j);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(x), j);
    return __hiloint2double(hi, lo);
}

__global__ __launch_bounds__(kRhokWaves * 64) void rhok_terms_kernel(RhokTermsArgs a)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int unit = blockIdx.x * kRhokWaves + wave;           // wave-uniform
    if (unit >= a.pchunks * a.mchunks) return;
    const int y = unit % a.mchunks, p = unit / a.mchunks;
    const int m = y * kRhokModeChunk + lane;
    const bool mode_live = m < a.n_modes;
    // a lane without a mode runs mode (0, 0, 0) and stores zeros into the padding of its row
    const double nx = mode_live ? (double)a.modes[3 * m] : 0.0;
    const double ny = mode_live ? (double)a.modes[3 * m + 1] : 0.0;
    const double nz = mode_live ? (double)a.modes[3 * m + 2] : 0.0;

    long long re_hi = 0, re_lo = 0, im_hi = 0, im_lo = 0;
    bool bad = false;
    const size_t P = (size_t)a.P;
    const int t0 = p * a.tiles, t1 = min(t0 + a.tiles, a.T);
    for (int t = t0; t < t1; ++t) {
        const size_t s = (size_t)t * kTile + lane;              // < T 64 <= P
        const int id = a.perm[s];
        const double tx = ljmdk::rhok_turns(a.pos[s], a.L);
        const double ty = ljmdk::rhok_turns(a.pos[P + s], a.L);
        const double tz = ljmdk::rhok_turns(a.pos[2 * P + s], a.L);
        unsigned long long live = __ballot(id >= 0 && id < a.n);
        while (live) {
            const int j = __builtin_ctzll(live);
            live &= live - 1;
            const double ux = lane_value(tx, j), uy = lane_value(ty, j), uz = lane_value(tz, j);
            double C, S;
            ljmdk::rhok_term(nx, ny, nz, ux, uy, uz, C, S);
            const bool oob = ljmdk::rhok_out_of_range(C, S);
            bad = bad || oob;
            long long h, l;
            ljmdk::rhok_fixed_parts(oob ? 0.0 : C, h, l);
            re_hi += h; re_lo += l;
            ljmdk::rhok_fixed_parts(oob ? 0.0 : S, h, l);
            im_hi += h; im_lo += l;
        }
    }
    uint64_t q[3];
    uint64_t *row = a.part + ((size_t)p * a.mchunks * kRhokModeChunk + m) * kRhokRowWords;
    from128(q, (__int128)re_hi * ((__int128)1 << 32) + (__int128)re_lo);
    row[0] = mode_live ? q[0] : 0; row[1] = mode_live ? q[1] : 0; row[2] = mode_live ? q[2] : 0;
    from128(q, (__int128)im_hi * ((__int128)1 << 32) + (__int128)im_lo);
    row[3] = mode_live ? q[0] : 0; row[4] = mode_live ? q[1] : 0; row[5] = mode_live ? q[2] : 0;
    const bool any_bad = __any(bad && mode_live);
    if (lane == 0) a.flag[(size_t)p * a.mchunks + y] = any_bad ? 1u : 0u;
}

__global__ __launch_bounds__(kRhokFoldWaves * 64) void rhok_fold_kernel(RhokFoldArgs a)
{
    __shared__ uint64_t wsum[kRhokFoldWaves][kRhokRowWords][64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int y = blockIdx.x;
    const int m = y * kRhokModeChunk + lane;
    uint64_t re[3] = {0, 0, 0}, im[3] = {0, 0, 0};
    unsigned bad = 0;
    for (int p = wave; p < a.pchunks; p += kRhokFoldWaves) {
        const uint64_t *src = a.part + ((size_t)p * a.mchunks * kRhokModeChunk + m) * kRhokRowWords;
        const uint64_t o0[3] = {src[0], src[1], src[2]}, o1[3] = {src[3], src[4], src[5]};
        add192(re, o0);
        add192(im, o1);
        bad |= a.flag[(size_t)p * a.mchunks + y];
    }
#pragma unroll
    for (int w = 0; w < 3; ++w) {
        wsum[wave][w][lane] = re[w];
        wsum[wave][3 + w][lane] = im[w];
    }
    const int any_bad = __syncthreads_or(bad != 0 ? 1 : 0);
    if (wave != 0) return;
    for (int k = 1; k < kRhokFoldWaves; ++k) {
        const uint64_t o0[3] = {wsum[k][0][lane], wsum[k][1][lane], wsum[k][2][lane]};
        const uint64_t o1[3] = {wsum[k][3][lane], wsum[k][4][lane], wsum[k][5][lane]};
        add192(re, o0);
        add192(im, o1);
    }
    if (m < a.n_modes) {
        uint64_t *dst = a.row + (size_t)m * kRhokRowWords;
#pragma unroll
        for (int w = 0; w < 3; ++w) {
            dst[w] = re[w];
            dst[3 + w] = im[w];
        }
    }
    if (any_bad && lane == 0) *a.range = 1;                     // every writer stores the same value
}

}  // namespace

hipError_t launch_rhok_terms(const RhokTermsArgs &a, hipStream_t s)
{
    if (!rhok_terms_ok(a)) return hipErrorInvalidValue;
    const int units = a.pchunks * a.mchunks;
    hipLaunchKernelGGL(rhok_terms_kernel, dim3((units + kRhokWaves - 1) / kRhokWaves), dim3(kRhokWaves * 64), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_rhok_fold(const RhokFoldArgs &a, hipStream_t s)
{
    if (!rhok_fold_ok(a)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rhok_fold_kernel, dim3(a.mchunks), dim3(kRhokFoldWaves * 64), 0, s, a);
    return hipGetLastError();
}

}  // namespace ljmdc
