// ljmd_batch_prepare.hip -- gfx950 kernels of the batch engine's on-device initial configurations (include/ljmd.h:
// ljmd_batch_prepare): one workgroup per replica, the launch geometry of the batch kernels (ljmd_batch.hip).
//
// batch_init_kernel, per replica of n = 4 k^3 particles in a box L (scripts/md_initial_config_program.f90:58-88):
//   lattice   : cells ix > iy > iz, four basis particles per cell; a = L / dble(k), x0 = dble(ix) * a, offsets
//               x0 + 0.5 * a -- the reference's expressions, unfused (-ffp-contract=off, csrc/Makefile)
//   velocities: the reference's generator (fortran/random_numbers.f90) on its integer state: particle i takes draws
//               3 i, 3 i + 1, 3 i + 2; a draw is double(m) * (1 / 4e6), v = draw - 0.5
//   centre of mass: per axis v_cm = R(sum_i Q(v_i)) / dble(n), the exact integer sum of the reproducible mode
//               (fixed_add, block_sum192: no summation order), v_i <- v_i - v_cm
// The generator is the only serial part.  Its table of 55 words is scattered and churned by thread 0 (274 integer
// steps); then x_j = x_{j-55} - x_{j-24} (mod 4 10^6) lets 24 lanes produce 24 consecutive draws per round.  The whole
// sequence stays in LDS -- 55 + 3 n words, x[55 + j] = x[j] - x[j + 31] -- so no index is taken modulo 55 and every
// thread then reads its own particles' draws from it.  One barrier per round: a round reads only what earlier rounds
// wrote (j + 31 < 55 + 24 r for every j of round r), and writes what no lane of the round reads.
// LDS: 4 (55 + 3 NMAX) bytes of draws, 1920 bytes of block_sum192, 24 bytes of v_cm.
//
// batch_scale_kernel: v <- v * scale[b].
#include "ljmd_batch_prepare.h"
#include "ljmd_internal.h"

namespace ljmdb {
namespace {

using ljmdk::block_sum192;
using ljmdk::fixed_add;
using ljmdk::fixed_to_double;
using ljmdk::from128;

// the table after random_uniform's first call with seed -|seed| has set it up, before any draw: x[p - 1] = table(p)
__device__ void ran_prime(int *x, int seed)
{
    const long long d = (long long)kRanSeedOffset - (seed < 0 ? -(long long)seed : (long long)seed);
    int cur = (int)((d < 0 ? -d : d) % kRanModulus);
    x[kRanTable - 1] = cur;
    int nxt = 1;
    for (int i = 1; i < kRanTable; ++i) {
        const int pos = (21 * i) % kRanTable;      // 1 .. 54: 55 does not divide 21 i
        x[pos - 1] = nxt;
        nxt = cur - nxt;
        if (nxt < 0) nxt += kRanModulus;
        cur = x[pos - 1];
    }
    for (int pass = 0; pass < 4; ++pass)
        for (int i = 1; i <= kRanTable; ++i) {
            int t = x[i - 1] - x[(i + 30) % kRanTable];
            if (t < 0) t += kRanModulus;
            x[i - 1] = t;
        }
}

// component ax of particle i's velocity before the centre of mass is removed: draw 3 i + ax of the sequence, - 0.5
__device__ __forceinline__ double ran_velocity(const int *x, int i, int ax)
{
    return (double)x[kRanTable + 3 * i + ax] * (1.0 / 4.0e6) - 0.5;
}

template <int NMAX, int K>
__global__ __launch_bounds__(kBatchMaxThreads) void batch_init_kernel(BatchInitArgs a)
{
    __shared__ int x[kRanTable + 3 * NMAX];           // the table, then the draws 0 .. 3 n - 1
    __shared__ uint64_t red[kBatchMaxWaves][5][3];
    __shared__ double vcm[3];
    const BatchReplica &rp = a.rep[a.g0 + blockIdx.x];
    const int n = rp.n <= NMAX ? rp.n : NMAX, T = rp.threads, tid = threadIdx.x;   // n <= NMAX by the class grouping
    const size_t plane = a.plane, base = rp.off;

    if (tid == 0) ran_prime(x, a.seeds[rp.b]);
    __syncthreads();
    const int draws = 3 * n;
    for (int j0 = 0; j0 < draws; j0 += kRanLanes) {   // uniform trip count: every thread meets every barrier
        const int j = j0 + tid;
        if (tid < kRanLanes && j < draws) {
            int t = x[j] - x[j + 31];
            if (t < 0) t += kRanModulus;
            x[kRanTable + j] = t;
        }
        __syncthreads();
    }

    // the centre of mass first, from the draws alone; the particles' values are formed again when they are stored, so
    // that nothing but the three sums lives across the reduction
    __int128 q[3] = {0, 0, 0};
    if (tid < T) {
#pragma unroll 1
        for (int i = tid; i < n; i += T)
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) fixed_add(q[ax], ran_velocity(x, i, ax));   // |v| <= 0.5: always in range
    }
    uint64_t w[5][3] = {};
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) from128(w[ax], q[ax]);
    block_sum192<true>(w, red, T >> 6);
    if (tid == 0)
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) vcm[ax] = fixed_to_double(w[ax]) / (double)n;
    __syncthreads();

    int cells = 1;                                    // k with 4 k^3 = n (the host has checked that there is one)
    while (4 * cells * cells * cells < n) ++cells;
    const double cell = rp.L / (double)cells;
    if (tid < T) {
#pragma unroll 1
        for (int i = tid; i < n; i += T) {
            const int c = i >> 2, basis = i & 3;
            const int ic[3] = {c / (cells * cells), (c / cells) % cells, c % cells};
            // basis 0: (0,0,0)  1: (0,1/2,1/2)  2: (1/2,0,1/2)  3: (1/2,1/2,0)
            const bool half[3] = {basis >= 2, basis == 1 || basis == 3, basis == 1 || basis == 2};
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {
                const double x0 = (double)ic[ax] * cell;
                const double r = half[ax] ? x0 + 0.5 * cell : x0;
                const size_t o = (size_t)ax * plane + base + i;
                a.state[o] = r;                                             // r
                a.state[3 * plane + o] = r;                                 // ru <- r
                a.state[6 * plane + o] = ran_velocity(x, i, ax) - vcm[ax];  // v
            }
        }
    }
}

template <int NMAX, int K>
__global__ __launch_bounds__(kBatchMaxThreads) void batch_scale_kernel(BatchScaleArgs a)
{
    const BatchReplica &rp = a.rep[a.g0 + blockIdx.x];
    const int n = rp.n, T = rp.threads, tid = threadIdx.x;
    if (tid >= T) return;
    const double s = a.scale[rp.b];
    double *const v = a.state + 6 * a.plane + rp.off;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int i = tid + k * T;
        if (i >= n) continue;
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) v[(size_t)ax * a.plane + i] = v[(size_t)ax * a.plane + i] * s;
    }
}

}  // namespace

hipError_t launch_batch_init(const BatchInitArgs &a, int n_max, int n_blocks, hipStream_t s)
{
    return dispatch_class(n_max, n_blocks, [&](auto nmax, auto k) {
        hipLaunchKernelGGL((batch_init_kernel<nmax(), k()>), dim3(n_blocks), dim3(batch_threads(n_max)), 0, s, a);
    });
}

hipError_t launch_batch_scale(const BatchScaleArgs &a, int n_max, int n_blocks, hipStream_t s)
{
    return dispatch_class(n_max, n_blocks, [&](auto nmax, auto k) {
        hipLaunchKernelGGL((batch_scale_kernel<nmax(), k()>), dim3(n_blocks), dim3(batch_threads(n_max)), 0, s, a);
    });
}

}  // namespace ljmdb
