// ljmd_batch_rhok.hip -- gfx950 kernel of the batch engine's density modes (include/ljmd.h: ljmd_batch_rhok_*): per
// replica b the sums of Q(cos k . r_j) and Q(sin k . r_j) over its n_b particles for every mode of the handle's list,
// from the replica's resident wrapped positions.  The arithmetic of a term is ljmd_rhok_arith.h, unfused
// (-ffp-contract=off, csrc/Makefile); every term enters an exact integer sum as Q(t) = RNE(t 2^64), so the words depend
// on no order: not on the particle order, the wave count or the grid.
//
// batch_rhok_kernel<W>   workgroup (x, y) = (table entry g0 + x, mode chunk y) owns its 64 modes of its replica
//                        completely.  Lane l keeps mode 64 y + l's triple and its two (hi, lo) int64 accumulators in
//                        registers.  The W waves share the replica's ceil(n_b / 64) tiles of 64 consecutive particles of
//                        its plane segment (rep.off), wave w taking tiles w, w + W, ...: lane l reduces particle l of the
//                        tile to turns (one division per coordinate and particle, not one per mode), and the wave walks the
//                        live lanes -- the ballot of index < n_b; the layout is contiguous, so there is no permutation and
//                        no padding slot -- taking the particle's three turns wave-uniform from lane j (v_readlane: no LDS,
//                        no barrier).  The waves meet once in LDS behind a barrier that every thread executes, a wave
//                        without a tile included; wave 0 adds the W partial rows and stores the six words of each live
//                        mode straight into row (snapshot, b, mode) of the series, whose only writer it is.  A term that is
//                        not finite enters as two zeros and sets the replica's sticky range word by a plain store of 1.
// One kernel for all five batch classes: nothing here scales with NMAX.  No global atomics, no floating-point atomics,
// no spin-waits, no dependency between workgroups, no scratch.
// Resources (make asm, -Rpass-analysis=kernel-resource-usage), W = 2 / 4 / 8: 50 / 50 / 58 VGPRs, 86 / 86 / 86 SGPRs,
// 4352 / 8448 / 16640 bytes of LDS, scratch 0, 8 waves per SIMD each.  W = 8 is the one launched (kBatchRhokWaves,
// profiles/batch_rhok_rate.txt); the other two are reached by LJMD_BATCH_RHOK_WAVES alone, for that measurement.
#include "ljmd_batch_rhok.h"

#include "ljmd_internal.h"
#include "ljmd_rhok_arith.h"

namespace ljmdb {
namespace {

using ljmdk::from128;

static_assert(kBatchRhokModeChunk == 64, "lane l stages particle l of a tile and owns mode l of a chunk");

// lane `j` (wave-uniform) of x, in SGPRs
__device__ __forceinline__ double lane_value(double x, int j)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(x), j);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(x), j);
    return __hiloint2double(hi, lo);
}

template <int W>
__global__ __launch_bounds__(W * 64) void batch_rhok_kernel(BatchRhokArgs a)
{
    __shared__ long long wsum[W][4][64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const BatchReplica rep = a.rep[a.g0 + blockIdx.x];
    const int m = blockIdx.y * kBatchRhokModeChunk + lane;
    const bool mode_live = m < a.n_modes;
    // a lane without a mode runs mode (0, 0, 0) and stores nothing
    const double nx = mode_live ? (double)a.modes[3 * m] : 0.0;
    const double ny = mode_live ? (double)a.modes[3 * m + 1] : 0.0;
    const double nz = mode_live ? (double)a.modes[3 * m + 2] : 0.0;

    long long re_hi = 0, re_lo = 0, im_hi = 0, im_lo = 0;
    bool bad = false;
    const double *rx = a.r + rep.off, *ry = rx + a.plane, *rz = ry + a.plane;
    const int tiles = (rep.n + 63) >> 6;
    for (int t = wave; t < tiles; t += W) {
        const int i = t * 64 + lane;
        const int ic = min(i, rep.n - 1);                       // a lane past the end loads the last particle and is not live
        const double tx = ljmdk::rhok_turns(rx[ic], rep.L);
        const double ty = ljmdk::rhok_turns(ry[ic], rep.L);
        const double tz = ljmdk::rhok_turns(rz[ic], rep.L);
        unsigned long long live = __ballot(i < rep.n);
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
    wsum[wave][0][lane] = re_hi;
    wsum[wave][1][lane] = re_lo;
    wsum[wave][2][lane] = im_hi;
    wsum[wave][3][lane] = im_lo;
    const int any_bad = __syncthreads_or(bad && mode_live ? 1 : 0);
    if (wave != 0) return;
    // at most 4096 parts below 2^34 in all: the int64 sums of the waves' sums are exact
#pragma unroll
    for (int k = 1; k < W; ++k) {
        re_hi += wsum[k][0][lane];
        re_lo += wsum[k][1][lane];
        im_hi += wsum[k][2][lane];
        im_lo += wsum[k][3][lane];
    }
    if (mode_live) {
        uint64_t *dst = a.words + (((size_t)a.row * a.B + (size_t)rep.b) * (size_t)a.n_modes + (size_t)m) * kBatchRhokRowWords;
        uint64_t q[3];
        from128(q, (__int128)re_hi * ((__int128)1 << 32) + (__int128)re_lo);
        dst[0] = q[0]; dst[1] = q[1]; dst[2] = q[2];
        from128(q, (__int128)im_hi * ((__int128)1 << 32) + (__int128)im_lo);
        dst[3] = q[0]; dst[4] = q[1]; dst[5] = q[2];
    }
    if (any_bad && lane == 0) a.range[rep.b] = 1;               // every writer stores the same value
}

template <int W>
hipError_t launch(const BatchRhokArgs &a, int n_blocks, hipStream_t s)
{
    const int mchunks = (a.n_modes + kBatchRhokModeChunk - 1) / kBatchRhokModeChunk;
    hipLaunchKernelGGL(batch_rhok_kernel<W>, dim3(n_blocks, mchunks), dim3(W * 64), 0, s, a);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_batch_rhok(const BatchRhokArgs &a, int n_blocks, int waves, hipStream_t s)
{
    if (!batch_rhok_ok(a, n_blocks, waves)) return hipErrorInvalidValue;
    switch (waves) {
    case 2: return launch<2>(a, n_blocks, s);
    case 4: return launch<4>(a, n_blocks, s);
    default: return launch<8>(a, n_blocks, s);
    }
}

}  // namespace ljmdb
