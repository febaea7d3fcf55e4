// ljmd_batch_heatflux.hip -- gfx950 kernel of the batch engine's heat flux (include/ljmd.h: ljmd_batch_heatflux_*): one
// snapshot -- the sums of phi w_a and g d_a over the pairs within the cutoff and of k2 v_a over the particles -- of every
// replica of a launch, one workgroup per replica.
//
// Per replica b, with its own n, L and rc, exactly the 9 integers of ljmd_heatflux_* (ljmd_heatflux.hip) for one system:
// the per-pair and per-particle arithmetic is the one copy of ljmd_heatflux_arith.h, the minimum image that of
// ljmd_stress_arith.h, Q(t) = RNE(t 2^64) and the 192-bit sums that of ljmd_sum192.h, compiled with -ffp-contract=off
// (csrc/Makefile).  Integer sums depend on no order: not on B, on the replica's slot, on the grouping into launches, on
// the streams, on the precision mode or on the order of the particles.
//
// Shape: batch_stress_kernel's (ljmd_batch_stress.hip).  A thread tid < T = batch_threads(n) owns particles tid,
// tid + T, ... (K of them), position and velocity of the one it is working on in registers; j is uniform across the wave,
// so every LDS read is a broadcast.  Every unordered pair is evaluated once (j > i: a wave starts j behind its first own
// particle) and the pair sums are doubled as integers: under i <-> j a pair's six terms keep their bits
// (ljmd_heatflux_arith.h).  The pair term needs the column particle's velocity, so the column operands are r and v: six
// planes in LDS, 96 KB for 2048 columns.  The 4096 class therefore walks its columns in two chunks of
// kBatchHeatfluxChunk with a barrier between, j > i and the wave's start rule applied inside each chunk; the other
// classes have one chunk and no such barrier.  Six 128-bit accumulators per thread run across its K passes (at most
// 4 * 4095 terms below 2^104), three more take the particle terms.  Then 192 bits (ljmd_sum192.h): integer shuffles
// across the wave, the replica's T / 64 waves through LDS after ONE barrier, and threads 0..8 store the 9 sums into the
// replica's row of the snapshot, which no other workgroup writes; the range flag is ORed into the replica's own sticky
// word by a plain store.
// No global atomics, no floating-point atomics, no spin-waits, no dependency between workgroups.
#include "ljmd_batch_heatflux.h"

#include "ljmd_heatflux_arith.h"
#include "ljmd_internal.h"
#include "ljmd_stress_arith.h"
#include "ljmd_sum192.h"

namespace ljmdb {
namespace {

using ljmdk::add_six;
using ljmdk::heatflux_add_kinetic;
using ljmdk::heatflux_terms;
using ljmdk::kHeatfluxKinTerms;
using ljmdk::kHeatfluxPairTerms;
using ljmdk::replica_lanes192;
using ljmdk::replica_rows192;
using ljmdk::stress_image;

static_assert(kBatchHeatfluxRows == kHeatfluxKinTerms + kHeatfluxPairTerms, "E[3], then P[3], C[3]");
static_assert(kBatchHeatfluxWords == kBatchHeatfluxRows * 3, "three limbs a sum");

// columns in LDS at a time, and the chunks a replica of the class has at most
constexpr int chunk_of(int nmax) { return nmax < kBatchHeatfluxChunk ? nmax : kBatchHeatfluxChunk; }
constexpr size_t lds_of(int nmax)
{
    return 6 * chunk_of(nmax) * sizeof(double) + kBatchMaxWaves * kBatchHeatfluxWords * sizeof(uint64_t);
}

template <int NMAX, int K>
__global__ __launch_bounds__(kBatchMaxThreads) void batch_heatflux_kernel(BatchHeatfluxArgs a)
{
    constexpr int CH = chunk_of(NMAX), NCHUNK = NMAX / CH;
    static_assert(NCHUNK * CH == NMAX, "whole chunks");
    __shared__ double col[6 * CH];          // x y z vx vy vz of the chunk's particles
    __shared__ uint64_t wsum[kBatchMaxWaves][kBatchHeatfluxRows][3];
    const BatchReplica &rp = a.rep[a.g0 + blockIdx.x];
    const int n = rp.n, T = rp.threads, tid = threadIdx.x;
    const double L = rp.L, invL = rp.invL, rc2 = rp.rc2;
    const size_t b = (size_t)rp.b;
    const size_t plane = a.plane, base = rp.off;
    const double *const R = a.state, *const V = a.state + 6 * plane;

    bool bad = false;
    __int128 pair[kHeatfluxPairTerms] = {0, 0, 0, 0, 0, 0}, kin[kHeatfluxKinTerms] = {0, 0, 0};
#pragma unroll
    for (int c = 0; c < NCHUNK; ++c) {
        const int c0 = c * CH;                              // block-uniform, as n is: every thread meets the barriers
        const int c1 = n < c0 + CH ? n : c0 + CH;
        if (c > 0) __syncthreads();                         // the last chunk has been read
        for (int j = c0 + tid; j < c1; j += blockDim.x) {
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {
                col[ax * CH + j - c0] = R[ax * plane + base + j];
                col[(3 + ax) * CH + j - c0] = V[ax * plane + base + j];
            }
        }
        __syncthreads();
        if (tid >= T) continue;     // wave-uniform (T is a multiple of 64); the waves from T on only join the barriers
#pragma unroll 1
        for (int k = 0; k < K; ++k) {
            const int i = tid + k * T;
            const bool live = i < n;        // an absent particle adds nothing: guarded by index, not by value
            const size_t gi = base + (live ? i : 0);
            const double xi = live ? R[gi] : 0.0, yi = live ? R[plane + gi] : 0.0, zi = live ? R[2 * plane + gi] : 0.0;
            const double vxi = live ? V[gi] : 0.0, vyi = live ? V[plane + gi] : 0.0, vzi = live ? V[2 * plane + gi] : 0.0;
            // the wave's first own particle of this pass: no j at or before it pairs with any of the wave's
            const int first = __builtin_amdgcn_readfirstlane((tid & ~63) + k * T) + 1;
            for (int j = first > c0 ? first : c0; j < c1; ++j) {
                const int s = j - c0;
                const double dx = stress_image(xi - col[s], L, invL);
                const double dy = stress_image(yi - col[CH + s], L, invL);
                const double dz = stress_image(zi - col[2 * CH + s], L, invL);
                const double r2 = dx * dx + dy * dy + dz * dz;
                if (live && j > i && r2 < rc2) {
                    double t[kHeatfluxPairTerms];
                    const bool oob = heatflux_terms(dx, dy, dz, r2, vxi + col[3 * CH + s], vyi + col[4 * CH + s],
                                                    vzi + col[5 * CH + s], t);
                    add_six(pair, t, oob, bad);
                }
            }
            if (c == 0 && live) heatflux_add_kinetic(kin, vxi, vyi, vzi, bad);
        }
    }

    if (tid < T) replica_lanes192(kin, pair, wsum);     // E[3], then P[3], C[3] with both orders of every pair
    replica_rows192(bad, T, wsum, a.words, a.row, a.B, b, a.range);
}

}  // namespace

hipError_t launch_batch_heatflux(const BatchHeatfluxArgs &a, int n_max, int n_blocks, hipStream_t s)
{
    // what the kernel's indexing rests on, beyond the replica table: a row inside the series
    if (!a.state || !a.words || !a.range || !a.rep || a.B < 1 || a.g0 < 0 || a.rows < 1 ||
        a.rows > kBatchHeatfluxMaxSnapshots || a.row < 0 || a.row >= a.rows)
        return hipErrorInvalidValue;
    return dispatch_class(n_max, n_blocks, [&](auto nmax, auto k) {
        static_assert(lds_of(nmax()) <= 160 * 1024, "LDS of one CU");
        hipLaunchKernelGGL((batch_heatflux_kernel<nmax(), k()>), dim3(n_blocks), dim3(batch_threads(n_max)), 0, s, a);
    });
}

}  // namespace ljmdb
