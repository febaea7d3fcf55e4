// ljmd_origins_dev.h -- the one copy of the device code that the kernels of the time-origin observables (ljmd_tcf.hip,
// ljmd_vanhove.hip) share: the gather kernel, the frame of a terms kernel -- the slice of a workgroup, its LDS entries,
// the current values of its particles, the walk over the ring slots, and the rows it writes -- and the fold kernel.
// Layout, constants and argument blocks: ljmd_origins.h.  Device code only.  No global atomics, no floating-point
// atomics, no spin-waits, no dependency between workgroups inside a launch.
#ifndef LJMD_ORIGINS_DEV_H
#define LJMD_ORIGINS_DEV_H

#include "ljmd_internal.h"
#include "ljmd_origins.h"

namespace ljmdk {

// slot order -> particle-id order through the DEVICE's permutation, the one scattered access; it also stores the snapshot
// into its ring slot when it becomes an origin (that slot's lag would be slots * stride > max_lag: no terms kernel reads it)
template <int C>
__global__ __launch_bounds__(kOriginThreads) void origin_gather_kernel(OriginGatherArgs a)
{
    static_assert(C == 3 || C == 6, "ru alone, or ru and v");
    const int s = blockIdx.x * kOriginThreads + threadIdx.x;
    if (s >= a.P) return;
    const int id = a.perm[s];
    if (id < 0 || id >= a.n) return;                // a padding slot
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const double x = c < 3 ? a.ru[(size_t)c * a.P + s] : a.v[(size_t)(c - 3) * a.P + s];
        a.cur[(size_t)c * a.n_pad + id] = x;
        if (a.store) a.store[(size_t)c * a.n_pad + id] = x;
    }
}

template <int C>
hipError_t launch_origin_gather(const OriginGatherArgs &a, hipStream_t s)
{
    if (!origin_gather_ok(a, C == 6)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(origin_gather_kernel<C>, dim3((a.P + kOriginThreads - 1) / kOriginThreads), dim3(kOriginThreads), 0, s, a);
    return hipGetLastError();
}

// The frame of a terms kernel, grid (particle blocks, origin slices); Args is the kernel's own argument block.

// the slice of this workgroup: origins e0 .. e0 + n_loc - 1, entries 0 .. n_ent - 1 of its LDS
struct OriginSlice {
    int e0, n_loc, n_ent;
    bool lag0;              // the newest origin is at lag 1 and belongs to this slice: its lag-0 terms go to entry n_loc
};

template <class Args>
__device__ __forceinline__ OriginSlice origin_slice(const Args &a)
{
    const int e0 = blockIdx.y * a.chunk, e1 = min(a.n_live, e0 + a.chunk), n_loc = e1 - e0;
    const bool lag0 = e1 == a.n_live && a.lag_first - (a.n_live - 1) * a.stride == 1;
    return {e0, n_loc, n_loc + (lag0 ? 1 : 0), lag0};
}

// acc[entries of the slice][2 kinds][2 words] = 0; the caller's barrier follows
__device__ __forceinline__ void origin_zero_entries(unsigned long long *acc, const OriginSlice &s)
{
    for (int k = threadIdx.x; k < 4 * s.n_ent; k += kOriginThreads) acc[k] = 0ull;
}

// index of the thread's first particle, ids i0 + k kOriginThreads: coalesced 8-byte loads
__device__ __forceinline__ size_t origin_first_id() { return (size_t)blockIdx.x * kOriginBlock + threadIdx.x; }

template <int C, class Args>
__device__ __forceinline__ void origin_load_current(const Args &a, double (&cur)[kOriginK][C])
{
    const size_t i0 = origin_first_id();
#pragma unroll
    for (int k = 0; k < kOriginK; ++k)
#pragma unroll
        for (int c = 0; c < C; ++c) cur[k][c] = a.cur[(size_t)c * a.n_pad + i0 + (size_t)k * kOriginThreads];
}

template <class Args>
__device__ __forceinline__ int origin_first_slot(const Args &a, const OriginSlice &s)
{
    return (a.slot_first + s.e0) % a.slots;
}

// the thread's elements of ring slot `slot` (component c of particle k: o[c n_pad + k kOriginThreads]); advances the slot
template <int C, class Args>
__device__ __forceinline__ const double *origin_next(const Args &a, int &slot)
{
    const double *const o = a.ring + (size_t)slot * C * a.n_pad + origin_first_id();
    slot = slot + 1 == a.slots ? 0 : slot + 1;
    return o;
}

// The end of a terms kernel, called by every thread: one barrier, behind which the entries are complete, then the
// entries e0 .. e0 + n_ent - 1 of this block's row of `part` (the lag-0 entry of the last slice is entry n_live) and the
// workgroup's range flag, by plain stores.
template <class Args>
__device__ __forceinline__ void origin_write_rows(const Args &a, const OriginSlice &s, const unsigned long long *acc, bool bad)
{
    const int any_bad = __syncthreads_or(bad ? 1 : 0);
    unsigned long long *const row = a.part + ((size_t)blockIdx.x * a.ents + s.e0) * 4;
    for (int k = threadIdx.x; k < 4 * s.n_ent; k += kOriginThreads) row[k] = acc[k];
    if (threadIdx.x == 0) a.flag[(size_t)blockIdx.x * a.slots + blockIdx.y] = any_bad;
}

// One thread per (entry, kind): adds the entry's partials over all particle blocks into sums[kind][lag] (the row's only
// writer; a workgroup's 1024 terms of one entry stay below 2^114, inside the 128-bit entry, and the fold adds in 192
// bits) and ORs the workgroups' range flags.  THREADS = kOriginThreads: a template so that the header defines it.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void origin_fold_kernel(OriginFoldArgs a)
{
    const int k = blockIdx.x * THREADS + threadIdx.x;
    const int n_live = a.n_live;
    const bool lag0 = a.lag_first - (n_live - 1) * a.stride == 1;
    const int n_ent = n_live + (lag0 ? 1 : 0);
    if (k >= 2 * n_ent) return;
    const int e = k >> 1, kind = k & 1;
    const int lag = e < n_live ? a.lag_first - e * a.stride : 0;
    if (lag < 0 || lag > a.max_lag) return;         // cannot happen with the host's arguments
    uint64_t tot[3] = {0, 0, 0};
    const unsigned long long *p = a.part + ((size_t)e * 2 + kind) * 2;
    for (int b = 0; b < a.nblk; ++b, p += (size_t)a.ents * 4) {
        const unsigned long long x0 = p[0], x1 = p[1];
        const uint64_t add[3] = {x0, x1, (long long)x1 < 0 ? ~0ull : 0ull};
        add192(tot, add);
    }
    uint64_t *const row = a.sums + ((size_t)kind * (a.max_lag + 1) + lag) * 3;
    uint64_t sum[3] = {row[0], row[1], row[2]};
    add192(sum, tot);
    row[0] = sum[0];
    row[1] = sum[1];
    row[2] = sum[2];
    // the flags of slice y: by the thread of the slice's first entry (the lag-0 entry belongs to the last slice)
    if (kind == 0 && e < n_live && e % a.chunk == 0) {
        const int slice = e / a.chunk;
        int bad = 0;
        for (int b = 0; b < a.nblk; ++b) bad |= a.flag[(size_t)b * a.slots + slice];
        if (bad) *a.range = 1;                      // every writer stores the same value
    }
}

inline hipError_t launch_origin_fold(const OriginFoldArgs &a, hipStream_t s)
{
    if (!origin_fold_ok(a)) return hipErrorInvalidValue;
    const int threads = 2 * (a.n_live + 1);
    hipLaunchKernelGGL(origin_fold_kernel<kOriginThreads>, dim3((threads + kOriginThreads - 1) / kOriginThreads),
                       dim3(kOriginThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace ljmdk
#endif
