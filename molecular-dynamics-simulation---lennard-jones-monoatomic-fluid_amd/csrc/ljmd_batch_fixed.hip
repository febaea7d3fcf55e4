// ljmd_batch_fixed.hip -- the batch kernel (ljmd_batch.hip) in the reproducible mode LJMD_PRECISION_FP64_REPRODUCIBLE:
// per replica exactly the contract of include/ljmd.h, bitwise equal to tests/reproducible_model.py and to a single
// reproducible engine, whatever B, the slot, the grouping into launches or the order of the particles.
//
// Structure as ljmd_batch.hip: one workgroup per replica, its positions SoA in LDS for the whole launch, j uniform
// across the workgroup, the replica table, the kernel classes and the three modes.  What differs:
//   pair term   = pair_fixed (ljmd_internal.h, the single engine's): round() minimum image, unfused r2, strict <,
//                 IEEE divide, fx = (m dx) u.  Every term enters a per-particle signed 128-bit sum as Q(t) = RNE(t 2^64);
//   kick        = fixed_tail_kernel: a = 24 R(particle sum) with ONE rounding, v += a dt/2, Q(v^2) per axis;
//   drift       = ljmd_batch.hip's, unchanged (drift_kick_kernel<0>, which the reproducible single engine uses too);
//   record      = kExactWords int64 per (sample, replica), the layout of ljmd_read_partials_exact: {S12, S6} over the
//                 ORDERED pairs (the host halves the integers), {Kx, Ky, Kz}, 192 bits each, and the flags word;
//   range       = a term that is not finite or has |t| >= 2^40 enters as 0 and sets the replica's sticky word in
//                 BatchFixedArgs::range (forces-only steps write no record, so the record's flag alone would not do).
// Integer sums are exact in any order: the thread count, the K mapping and the reduction tree are no part of the result.
//
// One own particle per pass over j (K passes per step): five 128-bit accumulators are 20 VGPRs, and a 1024-thread
// workgroup has 128 per lane.  A thread's S12 / S6 run on across its K passes (4 * 4095 terms of 2^104 < 2^118).
#include "ljmd_batch.h"
#include "ljmd_internal.h"

namespace ljmdb {
namespace {

using ljmdk::block_sum192;
using ljmdk::Drift;
using ljmdk::drift_wrap;
using ljmdk::fixed_add;
using ljmdk::fixed_out_of_range;
using ljmdk::fixed_to_double;
using ljmdk::from128;
using ljmdk::half_kick;
using ljmdk::kExactWords;
using ljmdk::kFlagNoEnergy;
using ljmdk::kFlagNoKinetic;
using ljmdk::kFlagRange;
using ljmdk::pair_fixed;

// thread 0: the exact record of (sample, replica)
__device__ __forceinline__ void write_record(int64_t *w, const uint64_t (&q)[5][3], int64_t flags)
{
#pragma unroll
    for (int k = 0; k < 5; ++k)
#pragma unroll
        for (int l = 0; l < 3; ++l) w[3 * k + l] = (int64_t)q[k][l];
    w[15] = flags;
}

// Q(v^2) of one velocity component into k; an out-of-range term enters as 0
__device__ __forceinline__ void kinetic_term(__int128 &k, double v, bool &bad)
{
    const double t = v * v;
    const bool oob = fixed_out_of_range(t);
    bad = bad || oob;
    fixed_add(k, oob ? 0.0 : t);
}

// all n positions of the replica against the own particle i; the next j's coordinates are read ahead of the pair
template <int NMAX, bool ENERGY>
__device__ __forceinline__ void gather_fixed(const double *pos, int n, double xi, double yi, double zi, int i, double L,
                                             double invL, double rc2, __int128 (&f)[3], __int128 &s12, __int128 &s6,
                                             bool &bad)
{
    f[0] = f[1] = f[2] = 0;
    double xj = pos[0], yj = pos[NMAX], zj = pos[2 * NMAX];
#pragma unroll 1
    for (int j = 0; j < n; ++j) {
        const int jn = j + 1 < n ? j + 1 : j;
        const double xn = pos[jn], yn = pos[NMAX + jn], zn = pos[2 * NMAX + jn];
        pair_fixed<ENERGY>(xi, yi, zi, xj, yj, zj, L, invL, rc2, j == i, f[0], f[1], f[2], s12, s6, bad);
        xj = xn;
        yj = yn;
        zj = zn;
    }
}

template <int NMAX, int K>
__global__ __launch_bounds__(kBatchMaxThreads) void batch_fixed_kernel(BatchFixedArgs fa)
{
    __shared__ double pos[3 * NMAX];
    __shared__ uint64_t red[kBatchMaxWaves][5][3];    // block_sum192 over the replica's T / 64 waves (the others hold zeros)
    const BatchArgs &a = fa.b;
    const BatchReplica &rp = a.rep[a.g0 + blockIdx.x];
    const int n = rp.n, T = rp.threads, tid = threadIdx.x;
    const double L = rp.L, invL = rp.invL, rc2 = rp.rc2, dt = rp.dt, dt_half = rp.dt_half, dt_sq_half = rp.dt_sq_half;
    const size_t b = (size_t)rp.b;
    const size_t plane = a.plane, base = rp.off;
    // own particles: i = tid + k T < n_own; an idle thread (tid >= T, whole waves) owns none
    const bool own = tid < T;
    const int n_own = own ? n : 0;
    double *const R = a.state;
    double *const RU = a.state + 3 * plane;
    double *const V = a.state + 6 * plane;
    double *const A = a.state + 9 * plane;
    bool bad = false;      // a term of this thread was out of range, at any step of the launch

    if (a.mode == kModeKinetic) {
        __int128 kq[3] = {0, 0, 0};
#pragma unroll 1
        for (int k = 0; k < K; ++k) {
            const int i = tid + k * T;
            if (i < n_own) {
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) kinetic_term(kq[ax], V[ax * plane + base + i], bad);
            }
        }
        uint64_t q[5][3] = {};
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) from128(q[2 + ax], kq[ax]);
        const bool any_bad = __syncthreads_or(bad);
        block_sum192<true>(q, red, T >> 6);
        if (tid == 0) {
            write_record(fa.rec + b * kExactWords, q, (any_bad ? kFlagRange : 0) | kFlagNoEnergy);
            if (any_bad) fa.range[b] = 1;
        }
        return;    // the mode is uniform across the launch: no thread of the workgroup reaches another barrier
    }

    for (int i = tid; i < n; i += blockDim.x) {
        pos[i] = R[base + i];
        pos[NMAX + i] = R[plane + base + i];
        pos[2 * NMAX + i] = R[2 * plane + base + i];
    }
    __syncthreads();

    const bool steps = a.mode == kModeSteps;
    const int nsteps = steps ? a.nsteps : 1;
    for (int s = 0; s < nsteps; ++s) {
        const int gstep = a.step0 + s + 1;
        const bool sampled = !steps || (a.sample_every > 0 && gstep % a.sample_every == 0);
        // the thread index again, opaque to the compiler: with K = 1 it would otherwise keep the 64-bit addresses of this
        // thread's elements of ru, v and a live across the pair loop, beyond the 128 VGPRs of a 1024-thread workgroup
        int ts = tid;
        asm volatile("" : "+v"(ts));
        if (steps) {
            // drift_kick_kernel<0>: r(t+dt), wrap, ru update, first half-kick (= ljmd_batch.hip)
#pragma unroll 1
            for (int k = 0; k < K; ++k) {
                const int i = ts + k * T;
                if (i < n_own) {
#pragma unroll
                    for (int ax = 0; ax < 3; ++ax) {
                        const size_t o = ax * plane + base + i;
                        const double v0 = V[o], acc = A[o];
                        const Drift h = drift_wrap(pos[ax * NMAX + i], v0, acc, dt, dt_sq_half, L, invL);
                        pos[ax * NMAX + i] = h.r1;
                        RU[o] = RU[o] + h.d;
                        V[o] = half_kick(v0, acc, dt_half);
                    }
                }
            }
            __syncthreads();
        }
        __int128 s12 = 0, s6 = 0, kq[3] = {0, 0, 0};      // this thread's totals of the step
        if (own) {     // wave-uniform (T is a multiple of 64); no barrier inside
#pragma unroll 1
            for (int k = 0; k < K; ++k) {
                const int i = ts + k * T;
                const bool have = i < n;
                const double xi = have ? pos[i] : __builtin_nan("");
                const double yi = have ? pos[NMAX + i] : __builtin_nan("");
                const double zi = have ? pos[2 * NMAX + i] : __builtin_nan("");
                __int128 f[3];
                if (sampled)
                    gather_fixed<NMAX, true>(pos, n, xi, yi, zi, i, L, invL, rc2, f, s12, s6, bad);
                else
                    gather_fixed<NMAX, false>(pos, n, xi, yi, zi, i, L, invL, rc2, f, s12, s6, bad);
                // fixed_tail_kernel: ONE rounding of the particle's integer sum, x24, second half-kick, Q(v^2) per axis
                if (have) {
#pragma unroll
                    for (int ax = 0; ax < 3; ++ax) {
                        const size_t o = ax * plane + base + i;
                        uint64_t w[3];
                        from128(w, f[ax]);
                        const double acc = 24.0 * fixed_to_double(w);
                        A[o] = acc;
                        if (steps) {
                            const double v1 = V[o] + acc * dt_half;
                            V[o] = v1;
                            kinetic_term(kq[ax], v1, bad);     // every step: the range test does not depend on sampling
                        }
                    }
                }
            }
        }
        if (sampled) {
            uint64_t q[5][3];
            from128(q[0], s12);
            from128(q[1], s6);
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) from128(q[2 + ax], kq[ax]);
            const bool any_bad = __syncthreads_or(bad);     // this or an earlier step of the launch
            block_sum192<true>(q, red, T >> 6);
            if (tid == 0) {
                const size_t rec = steps ? (size_t)(gstep / a.sample_every - 1) : 0;
                write_record(fa.rec + (rec * a.B + b) * kExactWords, q,
                             (any_bad ? kFlagRange : 0) | (steps ? 0 : kFlagNoKinetic));
            }
        }
        __syncthreads();   // every read of pos[] by this step's gather precedes the next drift's writes
    }
    if (__syncthreads_or(bad) && tid == 0) fa.range[b] = 1;
    if (steps) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int i = tid + k * T;
            if (i < n_own) {
                R[base + i] = pos[i];
                R[plane + base + i] = pos[NMAX + i];
                R[2 * plane + base + i] = pos[2 * NMAX + i];
            }
        }
    }
}

}  // namespace

hipError_t launch_batch_fixed(const BatchFixedArgs &a, int n_max, int n_blocks, hipStream_t s)
{
    return dispatch_class(n_max, n_blocks, [&](auto nmax, auto k) {
        hipLaunchKernelGGL((batch_fixed_kernel<nmax(), k()>), dim3(n_blocks), dim3(batch_threads(n_max)), 0, s, a);
    });
}

}  // namespace ljmdb
