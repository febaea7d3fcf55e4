// ljmd_batch.hip -- gfx950 kernel of the batch engine (include/ljmd.h: ljmd_batch_*): many independent small systems,
// each with its own (n, L, dt, rc), one workgroup per replica, many MD steps per launch.
//
// Per replica the arithmetic is the single engine's fast path, the very functions (ljmd_internal.h, last section):
//   drift + wrap + half-kick + unwrapped update  = drift_wrap, half_kick, as drift_kick_kernel<0> (ljmd_kernels.hip);
//   pair term                                    = pair_fast<true>, full-matrix gather form: every ordered pair
//                                                  (i, j != i), the energy sums scaled by 0.5 afterwards as the
//                                                  gather kernels' FinalizeArgs::pair_scale does;
//   second half-kick                             = kick_kernel<true>: a = 24 f, v += a dt/2, three separate sums of v^2.
// Compiled with -ffp-contract=off (csrc/Makefile): FMAs only where the source says fma().
//
// Determinism: every floating-point sum of a replica runs in an order fixed by its n alone -- j = 0 .. n-1 per particle,
// the own particles of a thread in order, the lanes of a wave by the shuffle tree, the waves in order.  Nothing
// depends on B, on the replica's slot or on the other replicas, and there are no floating-point atomics.  A replica
// reads its n and constants from the replica table (BatchReplica) and always uses its own thread count
// T = batch_threads(n) and mapping, whatever the launch's block size: a launch sized for a larger replica of the same
// class leaves the waves from T on idle, and they only take part in the barriers.
//
// Shape: the replica's positions stay in LDS (SoA, 3 NMAX doubles) for the whole launch; j is uniform across the
// workgroup, so every position read is a broadcast.  A thread tid < T owns particles tid, tid + T, ... (K of them); their
// ru, v, a stay in HBM (read and written by the owning thread only), their pair accumulators in registers.
#include "ljmd_batch.h"
#include "ljmd_internal.h"

namespace ljmdb {
namespace {

using ljmdk::block_sum;
using ljmdk::Drift;
using ljmdk::drift_wrap;
using ljmdk::half_kick;
using ljmdk::pair_fast;

// gather over all n positions of the replica for the K own particles of this thread
template <int NMAX, int K, bool ENERGY>
__device__ __forceinline__ void gather(const double *pos, int n, const double (&xi)[K], const double (&yi)[K],
                                       const double (&zi)[K], const int (&ii)[K], double L, double invL, double rc2,
                                       double (&f)[3][K], double (&e)[2][K])
{
#pragma unroll
    for (int k = 0; k < K; ++k) f[0][k] = f[1][k] = f[2][k] = e[0][k] = e[1][k] = 0.0;
#pragma unroll K == 1 ? 2 : 1
    for (int j = 0; j < n; ++j) {
        const double xj = pos[j], yj = pos[NMAX + j], zj = pos[2 * NMAX + j];
#pragma unroll
        for (int k = 0; k < K; ++k)
            pair_fast<true, ENERGY>(xi[k], yi[k], zi[k], xj, yj, zj, L, invL, rc2, j == ii[k],
                                    f[0][k], f[1][k], f[2][k], e[0][k], e[1][k]);
    }
}

template <int NMAX, int K>
__global__ __launch_bounds__(kBatchMaxThreads) void batch_md_kernel(BatchArgs a)
{
    __shared__ double pos[3 * NMAX];
    __shared__ double red[kBatchRecWords * kBatchMaxWaves];   // block_sum over the replica's own T / 64 waves
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

    if (a.mode == kModeKinetic) {
        double s[1] = {0.0};
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int i = tid + k * T;
            if (i < n_own) {
                const double vx = V[base + i], vy = V[plane + base + i], vz = V[2 * plane + base + i];
                s[0] += vx * vx + vy * vy + vz * vz;
            }
        }
        block_sum<1>(s, red, kBatchMaxWaves, T >> 6);
        if (tid == 0) {
            double *w = a.rec + b * kBatchRecWords;
            w[0] = 0.0;
            w[1] = 0.0;
            w[2] = s[0];
            w[3] = 0.0;
            w[4] = 0.0;
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
        if (steps) {
            // drift_kick_kernel<0>: r(t+dt), wrap, ru update, first half-kick
#pragma unroll 1
            for (int k = 0; k < K; ++k) {
                const int i = tid + k * T;
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
        // at most two own particles per pass over j (KG): four interleaved pair chains need more than the 128 VGPRs a
        // 1024-thread workgroup allows; a second pass costs only the LDS broadcasts.  The kick of a pass's particles
        // follows its pass, so nothing of it stays live.  Sums over the own particles run in order k = 0 .. K-1.
        constexpr int KG = K < 2 ? K : 2;
        double e12 = 0.0, e6 = 0.0, kk[3] = {0.0, 0.0, 0.0};
        if (own) {     // wave-uniform (T is a multiple of 64); no barrier inside
#pragma unroll 1
            for (int g = 0; g < K; g += KG) {
                double xs[KG], ys[KG], zs[KG], fs[3][KG], es[2][KG];
                int is[KG];
#pragma unroll
                for (int k = 0; k < KG; ++k) {
                    const int i = tid + (g + k) * T;
                    is[k] = i;
                    xs[k] = i < n ? pos[i] : __builtin_nan("");
                    ys[k] = i < n ? pos[NMAX + i] : __builtin_nan("");
                    zs[k] = i < n ? pos[2 * NMAX + i] : __builtin_nan("");
                }
                if (sampled)
                    gather<NMAX, KG, true>(pos, n, xs, ys, zs, is, L, invL, rc2, fs, es);
                else
                    gather<NMAX, KG, false>(pos, n, xs, ys, zs, is, L, invL, rc2, fs, es);
                // kick_kernel<KICK = steps>: a = 24 f, second half-kick, sums of v^2 per axis
#pragma unroll
                for (int k = 0; k < KG; ++k) {
                    if (is[k] < n) {
#pragma unroll
                        for (int ax = 0; ax < 3; ++ax) {
                            const size_t o = ax * plane + base + is[k];
                            const double acc = 24.0 * fs[ax][k];
                            A[o] = acc;
                            if (steps) {
                                const double v1 = V[o] + acc * dt_half;
                                V[o] = v1;
                                if (sampled) kk[ax] += v1 * v1;
                            }
                        }
                    }
                    e12 += es[0][k];
                    e6 += es[1][k];
                }
            }
        }
        if (sampled) {
            double v[kBatchRecWords] = {e12, e6, kk[0], kk[1], kk[2]};
            block_sum<kBatchRecWords>(v, red, kBatchMaxWaves, T >> 6);
            if (tid == 0) {
                const size_t rec = steps ? (size_t)(gstep / a.sample_every - 1) : 0;
                double *w = a.rec + (rec * a.B + b) * kBatchRecWords;
                w[0] = v[0] * 0.5;          // ordered -> unordered pairs; exact
                w[1] = v[1] * 0.5;
                w[2] = v[2];
                w[3] = v[3];
                w[4] = v[4];
            }
        }
        __syncthreads();   // every read of pos[] by this step's gather precedes the next drift's writes
    }
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

hipError_t launch_batch(const BatchArgs &a, int n_max, int n_blocks, hipStream_t s)
{
    return dispatch_class(n_max, n_blocks, [&](auto nmax, auto k) {
        hipLaunchKernelGGL((batch_md_kernel<nmax(), k()>), dim3(n_blocks), dim3(batch_threads(n_max)), 0, s, a);
    });
}

}  // namespace ljmdb
