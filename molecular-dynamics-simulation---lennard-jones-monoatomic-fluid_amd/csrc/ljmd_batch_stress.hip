// ljmd_batch_stress.hip -- gfx950 kernel of the batch engine's pressure tensor (include/ljmd.h: ljmd_batch_stress_*):
// one snapshot -- the six sums of f_a d_b over the pairs within the cutoff and of v_a v_b over the particles -- of every
// replica of a launch, one workgroup per replica.
//
// Per replica b, with its own n, L and rc, exactly the 12 integers of ljmd_stress_* (ljmd_stress.hip) for one system:
// the per-pair arithmetic and its range rule are the one copy of ljmd_stress_arith.h, Q(t) = RNE(t 2^64) and the 192-bit
// sums that of ljmd_sum192.h, compiled with -ffp-contract=off (csrc/Makefile).  Integer sums depend on no order: not on
// B, on the replica's slot, on the grouping into launches, on the streams, on the precision mode or on the order of the
// particles.
//
// Shape: batch_rdf_kernel's (ljmd_batch_rdf.hip).  The replica's positions are loaded once into LDS (SoA, 3 NMAX
// doubles); a thread tid < T = batch_threads(n) owns particles tid, tid + T, ... (K of them); j is uniform across the
// wave, so every position read is a broadcast.  Every unordered pair is evaluated once (j > i: a wave starts j behind its
// first own particle) and the virial sums are doubled as integers, as the one-rank walk of stress_pairs_kernel does.  Six
// 128-bit accumulators per thread run across its K passes (at most 4 * 4095 terms below 2^104); the same thread adds the
// six velocity products of its own particles into a second set.  Then 192 bits (ljmd_sum192.h): integer shuffles across
// the wave, the replica's T / 64 waves through LDS after ONE barrier, and threads 0..11 store the 12 sums into the replica's
// row of the snapshot, which no other workgroup writes; the range flag is ORed into the replica's own sticky word by a
// plain store.
// No global atomics, no floating-point atomics, no spin-waits, no dependency between workgroups.
#include "ljmd_batch_stress.h"

#include "ljmd_internal.h"
#include "ljmd_stress_arith.h"
#include "ljmd_sum192.h"

namespace ljmdb {
namespace {

using ljmdk::add_six;
using ljmdk::kStressTerms;
using ljmdk::replica_lanes192;
using ljmdk::replica_rows192;
using ljmdk::stress_image;
using ljmdk::stress_terms;

static_assert(kBatchStressWords == 2 * kStressTerms * 3, "K[6][3], then S[6][3]");

template <int NMAX, int K>
__global__ __launch_bounds__(kBatchMaxThreads) void batch_stress_kernel(BatchStressArgs a)
{
    __shared__ double pos[3 * NMAX];
    __shared__ uint64_t wsum[kBatchMaxWaves][2 * kStressTerms][3];
    const BatchReplica &rp = a.rep[a.g0 + blockIdx.x];
    const int n = rp.n, T = rp.threads, tid = threadIdx.x;
    const double L = rp.L, invL = rp.invL, rc2 = rp.rc2;
    const size_t b = (size_t)rp.b;
    const size_t plane = a.plane, base = rp.off;
    const double *const R = a.state, *const V = a.state + 6 * plane;

    for (int i = tid; i < n; i += blockDim.x) {
        pos[i] = R[base + i];
        pos[NMAX + i] = R[plane + base + i];
        pos[2 * NMAX + i] = R[2 * plane + base + i];
    }
    __syncthreads();

    bool bad = false;
    if (tid < T) {     // wave-uniform (T is a multiple of 64); the waves from T on only join the barriers
        __int128 vir[kStressTerms] = {0, 0, 0, 0, 0, 0}, kin[kStressTerms] = {0, 0, 0, 0, 0, 0};
#pragma unroll 1
        for (int k = 0; k < K; ++k) {
            const int i = tid + k * T;
            const bool live = i < n;        // an absent particle adds nothing: guarded by index, not by value
            const double xi = live ? pos[i] : 0.0, yi = live ? pos[NMAX + i] : 0.0, zi = live ? pos[2 * NMAX + i] : 0.0;
            // the wave's first own particle of this pass: no j at or before it pairs with any of the wave's
            const int j0 = __builtin_amdgcn_readfirstlane((tid & ~63) + k * T) + 1;
            for (int j = j0; j < n; ++j) {
                const double dx = stress_image(xi - pos[j], L, invL);
                const double dy = stress_image(yi - pos[NMAX + j], L, invL);
                const double dz = stress_image(zi - pos[2 * NMAX + j], L, invL);
                const double r2 = dx * dx + dy * dy + dz * dz;
                if (live && j > i && r2 < rc2) {
                    double t[kStressTerms];
                    const bool oob = stress_terms(dx, dy, dz, r2, t);
                    add_six(vir, t, oob, bad);
                }
            }
            if (live) {
                const double vx = V[base + i], vy = V[plane + base + i], vz = V[2 * plane + base + i];
                const double t[kStressTerms] = {vx * vx, vy * vy, vz * vz, vx * vy, vx * vz, vy * vz};
                add_six(kin, t, false, bad);
            }
        }
        replica_lanes192(kin, vir, wsum);       // K[6], then S[6] with both orders of every pair
    }
    replica_rows192(bad, T, wsum, a.words, a.row, a.B, b, a.range);
}

}  // namespace

hipError_t launch_batch_stress(const BatchStressArgs &a, int n_max, int n_blocks, hipStream_t s)
{
    // what the kernel's indexing rests on, beyond the replica table: a row inside the series
    if (!a.state || !a.words || !a.range || !a.rep || a.B < 1 || a.g0 < 0 || a.rows < 1 || a.rows > kBatchStressMaxSnapshots ||
        a.row < 0 || a.row >= a.rows)
        return hipErrorInvalidValue;
    return dispatch_class(n_max, n_blocks, [&](auto nmax, auto k) {
        static_assert(3 * nmax() * sizeof(double) + kBatchMaxWaves * kBatchStressWords * sizeof(uint64_t) <= 160 * 1024,
                      "LDS of one CU");
        hipLaunchKernelGGL((batch_stress_kernel<nmax(), k()>), dim3(n_blocks), dim3(batch_threads(n_max)), 0, s, a);
    });
}

}  // namespace ljmdb
