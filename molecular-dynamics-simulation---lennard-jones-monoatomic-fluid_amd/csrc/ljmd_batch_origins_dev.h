// ljmd_batch_origins_dev.h -- the one copy of the device code that the kernels of the batch engine's time-origin
// observables (ljmd_batch_tcf.hip, ljmd_batch_vanhove.hip) share: the frame of a workgroup -- its replica and its LDS
// entries --, an element of the current snapshot, the walk over the ring slots, the store of the snapshot as an origin,
// and the rows the workgroup adds its entries to.  Argument block and window: BatchOriginArgs (ljmd_batch.h).  What an
// origin contributes and where the barriers stand is each kernel's own.  Device code only.  No global atomics, no
// floating-point atomics, no spin-waits.
// The current snapshot is shared per element: filled as an array in one shared function and stored from another, it
// became one vector value, and batch_tcf_kernel<2048, 2> went from 68 VGPRs and 7 waves per SIMD to 76 and 6.
#ifndef LJMD_BATCH_ORIGINS_DEV_H
#define LJMD_BATCH_ORIGINS_DEV_H

#include "ljmd_batch.h"
#include "ljmd_internal.h"

namespace ljmdb {

// The workgroup's replica, read once, and its LDS entries: 0 .. n_live - 1 belong to the live origins, entry n_live takes
// the lag-0 terms.  A thread tid < T owns particles tid, tid + T, ...
struct BatchOriginFrame {
    int n, T, b;            // the replica's particles, threads and index
    size_t base;            // its first element in every plane
    int n_live, n_ent;
    bool lag0;              // the newest origin is at lag 1
};

// acc[n_ent][2 kinds][2 words] = 0; the caller's barrier follows
__device__ __forceinline__ BatchOriginFrame batch_origin_frame(const BatchOriginArgs &a, unsigned long long *acc)
{
    const BatchReplica &rp = a.rep[a.g0 + blockIdx.x];
    const int n_live = a.n_live;
    const bool lag0 = n_live > 0 && a.lag_first - (n_live - 1) * a.stride == 1;
    const int n_ent = n_live + (lag0 ? 1 : 0);
    for (int k = threadIdx.x; k < 4 * n_ent; k += blockDim.x) acc[k] = 0ull;
    return {rp.n, rp.threads, rp.b, rp.off, n_live, n_ent, lag0};
}

// component c (0..2: ru, 3..5: v) of the current snapshot of the thread's particle k, tid + k T: planes 3 .. 8 of the
// state; 0 past the replica's n and for a thread that owns nothing
__device__ __forceinline__ double batch_origin_current(const BatchOriginArgs &a, const BatchOriginFrame &f, bool own, int k, int c)
{
    const int i = (int)threadIdx.x + k * f.T;
    return own && i < f.n ? a.state[(size_t)(3 + c) * a.plane + f.base + i] : 0.0;
}

// the replica's elements of ring slot `slot` (component c of particle i: o[c plane + i]); advances the slot
template <int C>
__device__ __forceinline__ const double *batch_origin_next(const BatchOriginArgs &a, const BatchOriginFrame &f, int &slot)
{
    const double *const o = a.ring + (size_t)slot * C * a.plane + f.base;
    slot = slot + 1 == a.slots ? 0 : slot + 1;
    return o;
}

// the snapshot becomes an origin: the slot's lag would be slots * stride > max_lag, so no live origin of this launch is
// in it, and a thread touches only its own particles' elements.  For the threads that own particles.
template <int C, int K>
__device__ __forceinline__ void batch_origin_store(const BatchOriginArgs &a, const BatchOriginFrame &f, const double (&cur)[K][C])
{
    if (a.store_slot < 0) return;
    double *const o = a.ring + (size_t)a.store_slot * C * a.plane + f.base;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int i = (int)threadIdx.x + k * f.T;
        if (i < f.n)
#pragma unroll
            for (int c = 0; c < C; ++c) o[(size_t)c * a.plane + i] = cur[k][c];
    }
}

// The end of a kernel, behind the barrier that completes the entries: the workgroup adds them into its own rows of the
// 192-bit sums with plain loads, add192 and stores -- it is the rows' only writer, and launches on one stream follow one
// another.
__device__ __forceinline__ void batch_origin_add_rows(const BatchOriginArgs &a, const BatchOriginFrame &f,
                                                      const unsigned long long *acc)
{
    const int rows = a.max_lag + 1;
    for (int k = threadIdx.x; k < 2 * f.n_ent; k += blockDim.x) {
        const int e = k >> 1, kind = k & 1;
        const int lag = e < f.n_live ? a.lag_first - e * a.stride : 0;
        if (lag < 0 || lag >= rows) continue;     // cannot happen with the host's arguments
        const unsigned long long x0 = acc[4 * e + 2 * kind], x1 = acc[4 * e + 2 * kind + 1];
        const uint64_t add[3] = {x0, x1, (long long)x1 < 0 ? ~0ull : 0ull};
        uint64_t *const row = a.sums + (((size_t)f.b * 2 + kind) * rows + lag) * 3;
        uint64_t sum[3] = {row[0], row[1], row[2]};
        ljmdk::add192(sum, add);
        row[0] = sum[0];
        row[1] = sum[1];
        row[2] = sum[2];
    }
}

}  // namespace ljmdb
#endif
