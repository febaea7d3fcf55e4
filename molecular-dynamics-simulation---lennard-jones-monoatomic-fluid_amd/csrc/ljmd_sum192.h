// ljmd_sum192.h -- the one copy of the exact 192-bit sums on the device, shared by the kernels of the series observables
// (ljmd_stress.hip, ljmd_heatflux.hip, ljmd_batch_stress.hip, ljmd_batch_heatflux.hip): a group of terms into 128-bit
// lane accumulators under the range rule, lanes -> wave -> LDS -> one row per workgroup (or per replica) by plain stores
// with the range flag, the frame of a kinetic kernel, and the fold kernel that adds the rows of one accumulate into a row
// of the series.  Q(t) = RNE(t 2^64), add192 and from128 are ljmd_internal.h's.  Device code only: the argument blocks
// and the launch guards are ljmd_series.h.  No global atomics, no floating-point atomics, no spin-waits, no dependency
// between workgroups.
#ifndef LJMD_SUM192_H
#define LJMD_SUM192_H

#include "ljmd_internal.h"
#include "ljmd_series.h"

namespace ljmdk {

// sum over the wave of one signed 192-bit integer per lane; valid in lane 0
__device__ __forceinline__ void wave_sum192(uint64_t (&q)[3])
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        uint64_t o[3];
#pragma unroll
        for (int w = 0; w < 3; ++w) o[w] = __shfl_down(q[w], off, 64);
        add192(q, o);
    }
}

// acc[c] += Q(t[c]) for the six terms -- or six zeros, and the flag, when `oob` or one of the terms is out of range
__device__ __forceinline__ void add_six(__int128 (&acc)[6], const double (&t)[6], bool oob, bool &bad)
{
#pragma unroll
    for (int c = 0; c < 6; ++c) oob = oob || fixed_out_of_range(t[c]);
    bad = bad || oob;
#pragma unroll
    for (int c = 0; c < 6; ++c) fixed_add(acc[c], oob ? 0.0 : t[c]);
}

// lanes -> wave: the N lane accumulators in 192 bits (64 lanes of 2^127, doubled, do not fit 128), `doubled` for both
// orders of every pair, summed over the wave; lane 0 leaves sum c in dst[c]
template <int N>
__device__ __forceinline__ void lanes_to_lds192(const __int128 (&acc)[N], bool doubled, int lane, uint64_t (*dst)[3])
{
#pragma unroll
    for (int c = 0; c < N; ++c) {
        uint64_t q[3];
        from128(q, acc[c]);
        if (doubled) {
            const uint64_t o[3] = {q[0], q[1], q[2]};
            add192(q, o);
        }
        wave_sum192(q);
        if (lane == 0) {
            dst[c][0] = q[0];
            dst[c][1] = q[1];
            dst[c][2] = q[2];
        }
    }
}

// waves -> row: sum c of the first `waves` rows of wsum into dst[0..2]
template <int ROWS>
__device__ __forceinline__ void waves_to_row192(const uint64_t (*wsum)[ROWS][3], int waves, int c, uint64_t *dst)
{
    uint64_t q[3] = {wsum[0][c][0], wsum[0][c][1], wsum[0][c][2]};
    for (int w = 1; w < waves; ++w) {
        const uint64_t o[3] = {wsum[w][c][0], wsum[w][c][1], wsum[w][c][2]};
        add192(q, o);
    }
    dst[0] = q[0];
    dst[1] = q[1];
    dst[2] = q[2];
}

// A workgroup of WAVES waves, this thread lane `lane` of wave `wave`: every thread's N accumulators -> ONE 192-bit sum per
// component in part[row][N][3] and the range flag in flag[row], the workgroup's own row, by plain stores of threads 0..N.
// Every thread of the workgroup calls it; it holds the one barrier, so what the caller left in LDS before the call is
// complete behind it.
template <int N, int WAVES>
__device__ __forceinline__ void workgroup_sum192(const __int128 (&acc)[N], bool doubled, const bool &bad, int lane, int wave,
                                                 uint64_t (&wsum)[WAVES][N][3], uint64_t *part, unsigned *flag, size_t row)
{
    lanes_to_lds192<N>(acc, doubled, lane, wsum[wave]);
    const int any_bad = __syncthreads_or(bad ? 1 : 0);
    if (threadIdx.x < N)
        waves_to_row192<N>(wsum, WAVES, threadIdx.x, part + (row * N + threadIdx.x) * 3);
    else if (threadIdx.x == N)
        flag[row] = any_bad ? 1u : 0u;
}

// A replica of the batch engine, the same operation with another destination, in two steps because only the threads
// [0, T) of its workgroup are live (T a multiple of 64).  A live thread: its KIN particle sums, then its PAIR pair sums
// with both orders of every pair, over its wave into wsum.
template <int KIN, int PAIR, int WAVES>
__device__ __forceinline__ void replica_lanes192(const __int128 (&kin)[KIN], const __int128 (&pair)[PAIR],
                                                 uint64_t (&wsum)[WAVES][KIN + PAIR][3])
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    lanes_to_lds192<KIN>(kin, false, lane, wsum[wave]);
    lanes_to_lds192<PAIR>(pair, true, lane, wsum[wave] + KIN);
}

// Every thread of the workgroup, with the one barrier inside: the replica's T / 64 waves into words[snapshot][b][ROWS][3]
// of the B replicas' series, a row which no other workgroup writes; the range flag is ORed into the replica's own sticky
// word range[b] by a plain store.
template <int ROWS, int WAVES>
__device__ __forceinline__ void replica_rows192(const bool &bad, int T, uint64_t (&wsum)[WAVES][ROWS][3], uint64_t *words,
                                                int64_t snapshot, size_t B, size_t b, int32_t *range)
{
    const int tid = threadIdx.x;
    const int any_bad = __syncthreads_or(bad ? 1 : 0);
    if (tid < ROWS)
        waves_to_row192<ROWS>(wsum, T / 64, tid, words + (((size_t)snapshot * B + b) * ROWS + tid) * 3);
    else if (tid == ROWS && any_bad)
        range[b] = 1;
}

// The frame of a kinetic kernel: THREADS threads, PER slots of v[3][P] each, add(acc, vx, vy, vz, bad) per slot (a padding
// slot holds 0: Q(0) = 0), then the workgroup's N sums and its flag into row blockIdx.x of kpart / kflag.
template <int N, int THREADS, int PER, class Add>
__device__ __forceinline__ void series_kinetic(const SeriesKineticArgs &a, Add &&add)
{
    __shared__ uint64_t wsum[THREADS / 64][N][3];
    __int128 acc[N] = {};
    bool bad = false;
    const size_t P = (size_t)a.P;
    const size_t s0 = (size_t)blockIdx.x * (THREADS * PER) + threadIdx.x;
#pragma unroll 1
    for (int k = 0; k < PER; ++k) {
        const size_t s = s0 + (size_t)k * THREADS;
        if (s >= P) break;
        add(acc, a.v[s], a.v[P + s], a.v[2 * P + s], bad);
    }
    workgroup_sum192<N, THREADS / 64>(acc, false, bad, threadIdx.x & 63, threadIdx.x >> 6, wsum, a.kpart, a.kflag, blockIdx.x);
}

// One workgroup, one wave per output row: adds the partials in 192 bits, writes row s of the series (its only writer) --
// the KIN particle sums, then the PAIR pair sums -- the tile-pair counts of this accumulate (the last wave), and ORs the
// flags into the sticky word.
template <int KIN, int PAIR>
__global__ __launch_bounds__((KIN + PAIR + 1) * 64) void series_fold_kernel(SeriesFoldArgs a)
{
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);      // output row of this wave
    if (w < KIN + PAIR) {
        const bool kin = w < KIN;
        const int c = kin ? w : w - KIN;
        const int stride = kin ? KIN : PAIR;
        const uint64_t *src = kin ? a.kpart : a.part;
        const unsigned *flg = kin ? a.kflag : a.pflag;
        const int rows = kin ? a.blocks : a.workgroups;
        uint64_t q[3] = {0, 0, 0};
        unsigned bad = 0;
        for (int r = lane; r < rows; r += 64) {
            const uint64_t *p = src + ((size_t)r * stride + c) * 3;
            const uint64_t o[3] = {p[0], p[1], p[2]};
            add192(q, o);
            bad |= flg[r];
        }
        wave_sum192(q);
        const bool any_bad = __any(bad != 0);
        if (lane == 0) {
            uint64_t *dst = a.row + (size_t)w * 3;
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

template <int KIN, int PAIR>
hipError_t launch_series_fold(const SeriesFoldArgs &a, hipStream_t s)
{
    if (!series_fold_ok(a)) return hipErrorInvalidValue;
    hipLaunchKernelGGL((series_fold_kernel<KIN, PAIR>), dim3(1), dim3((KIN + PAIR + 1) * 64), 0, s, a);
    return hipGetLastError();
}

}  // namespace ljmdk
#endif
