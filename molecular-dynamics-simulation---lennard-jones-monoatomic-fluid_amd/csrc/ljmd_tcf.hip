// ljmd_tcf.hip -- gfx950 kernels of the MSD / VACF accumulation of the system resident on a one-rank engine
// (include/ljmd.h: ljmd_tcf_*; layout and argument blocks: ljmd_tcf.h).  The definition is the batch engine's
// (ljmd_batch_tcf.hip) with B = 1, and the per-term arithmetic is the same code (ljmd_tcf_arith.h):
//   MSD : d = ru(s) - ru(t0) per axis ; t = (dx*dx + dy*dy) + dz*dz
//   VACF: t = (vx(s)*vx(t0) + vy(s)*vy(t0)) + vz(s)*vz(t0)            (-ffp-contract=off, csrc/Makefile)
// each entering an exact integer sum as Q(t) = RNE(t 2^64).  Integer sums depend on no order, so the result does not
// depend on the slot order, on the grid or on how the three kernels split the work.
//
// No pair loop: the path streams, its bound is HBM bandwidth -- 48 n_pad bytes per live origin.
//   1. tcf_gather_kernel  slot order -> particle-id order, through the DEVICE's permutation: the one scattered access
//                         (48 n bytes); it also stores the snapshot into its ring slot when it becomes an origin (that
//                         slot's lag would be slots * stride > max_lag: the terms kernel does not read it).
//   2. tcf_terms_kernel   grid (particle blocks, origin slices).  A thread keeps the current six values of its kTcfK
//                         particles (ids block * 1024 + tid + k 256: coalesced 8-byte loads) in registers and, per live
//                         origin of its slice, loads its own elements of the ring slot and forms the two terms (and the
//                         lag-0 terms of the newest origin when that is at lag 1).  Limbs are summed over the wave by
//                         integer shuffles, lane 0 adds the wave's 128-bit total into the origin's LDS entry; after ONE
//                         barrier the workgroup writes its entries with plain stores into its own rows of `part`.
//   3. tcf_fold_kernel    one thread per (entry, kind): adds the entry's partials over all particle blocks into
//                         sums[kind][lag] (the row's only writer) and ORs the workgroups' range flags.
// No global atomics, no floating-point atomics, no spin-waits, no dependency between workgroups inside a launch.
// A workgroup's 1024 terms of one entry stay below 2^114, inside the 128-bit entry; the fold adds in 192 bits.
#include "ljmd_tcf.h"

#include "ljmd_internal.h"
#include "ljmd_tcf_arith.h"

namespace ljmdt {
namespace {

using ljmdk::add192;
using ljmdk::entry_add;
using ljmdk::tcf_add;
using ljmdk::wave_sum_i64;

__global__ __launch_bounds__(kTcfThreads) void tcf_gather_kernel(TcfGatherArgs a)
{
    const int s = blockIdx.x * kTcfThreads + threadIdx.x;
    if (s >= a.P) return;
    const int id = a.perm[s];
    if (id < 0 || id >= a.n) return;                // a padding slot
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        const double x = c < 3 ? a.ru[(size_t)c * a.P + s] : a.v[(size_t)(c - 3) * a.P + s];
        a.cur[(size_t)c * a.n_pad + id] = x;
        if (a.store) a.store[(size_t)c * a.n_pad + id] = x;
    }
}

__global__ __launch_bounds__(kTcfThreads) void tcf_terms_kernel(TcfTermsArgs a)
{
    __shared__ unsigned long long acc[(kTcfMaxChunk + 1) * 4];     // [origins of the slice (+ 1)][2 kinds][2 words]
    const int tid = threadIdx.x, lane = tid & 63;
    const int blk = blockIdx.x, slice = blockIdx.y;
    const int n_live = a.n_live;
    const int e0 = slice * a.chunk, e1 = min(n_live, e0 + a.chunk), n_loc = e1 - e0;
    // the newest origin is at lag 1 and belongs to this slice: its lag-0 terms go to the entry behind the slice's
    const bool lag0 = e1 == n_live && a.lag_first - (n_live - 1) * a.stride == 1;
    const int n_ent = n_loc + (lag0 ? 1 : 0);

    for (int k = tid; k < 4 * n_ent; k += kTcfThreads) acc[k] = 0ull;
    __syncthreads();

    const size_t np = a.n_pad, i0 = (size_t)blk * kTcfBlock + tid;
    double cur[kTcfK][6];
#pragma unroll
    for (int k = 0; k < kTcfK; ++k)
#pragma unroll
        for (int c = 0; c < 6; ++c) cur[k][c] = a.cur[(size_t)c * np + i0 + (size_t)k * kTcfThreads];

    bool bad = false;
    int slot = (a.slot_first + e0) % a.slots;
#pragma unroll 1
    for (int e = 0; e < n_loc; ++e) {
        const double *const o = a.ring + (size_t)slot * 6 * np + i0;
        slot = slot + 1 == a.slots ? 0 : slot + 1;
        const bool with0 = lag0 && e == n_loc - 1;
        long long m_hi = 0, m_lo = 0, c_hi = 0, c_lo = 0;       // MSD and VACF limbs of this origin
        long long z_hi = 0, z_lo = 0, w_hi = 0, w_lo = 0;       // ... and of its lag 0
#pragma unroll
        for (int k = 0; k < kTcfK; ++k) {
            double org[6];
#pragma unroll
            for (int c = 0; c < 6; ++c) org[c] = o[(size_t)c * np + (size_t)k * kTcfThreads];
            const double dx = cur[k][0] - org[0], dy = cur[k][1] - org[1], dz = cur[k][2] - org[2];
            tcf_add(m_hi, m_lo, (dx * dx + dy * dy) + dz * dz, bad);
            tcf_add(c_hi, c_lo, (cur[k][3] * org[3] + cur[k][4] * org[4]) + cur[k][5] * org[5], bad);
            if (with0) {                                         // uniform across the workgroup
                const double ex = org[0] - org[0], ey = org[1] - org[1], ez = org[2] - org[2];
                tcf_add(z_hi, z_lo, (ex * ex + ey * ey) + ez * ez, bad);
                tcf_add(w_hi, w_lo, (org[3] * org[3] + org[4] * org[4]) + org[5] * org[5], bad);
            }
        }
        m_hi = wave_sum_i64(m_hi);
        m_lo = wave_sum_i64(m_lo);
        c_hi = wave_sum_i64(c_hi);
        c_lo = wave_sum_i64(c_lo);
        if (with0) {
            z_hi = wave_sum_i64(z_hi);
            z_lo = wave_sum_i64(z_lo);
            w_hi = wave_sum_i64(w_hi);
            w_lo = wave_sum_i64(w_lo);
        }
        if (lane == 0) {
            entry_add(acc + 4 * e, m_hi, m_lo);
            entry_add(acc + 4 * e + 2, c_hi, c_lo);
            if (with0) {
                entry_add(acc + 4 * n_loc, z_hi, z_lo);
                entry_add(acc + 4 * n_loc + 2, w_hi, w_lo);
            }
        }
    }
    const int any_bad = __syncthreads_or(bad ? 1 : 0);          // the one barrier: the entries are complete behind it

    // entries e0 .. e0 + n_ent - 1 of this block's row: the lag-0 entry of the last slice is entry n_live
    unsigned long long *const row = a.part + ((size_t)blk * a.ents + e0) * 4;
    for (int k = tid; k < 4 * n_ent; k += kTcfThreads) row[k] = acc[k];
    if (tid == 0) a.flag[(size_t)blk * a.slots + slice] = any_bad;
}

__global__ __launch_bounds__(kTcfThreads) void tcf_fold_kernel(TcfFoldArgs a)
{
    const int k = blockIdx.x * kTcfThreads + threadIdx.x;
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

}  // namespace

hipError_t launch_tcf_gather(const TcfGatherArgs &a, hipStream_t s)
{
    if (!a.ru || !a.v || !a.perm || !a.cur || a.n < 1 || a.P < a.n || a.n_pad < (size_t)a.n || a.n_pad % kTcfBlock != 0)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(tcf_gather_kernel, dim3((a.P + kTcfThreads - 1) / kTcfThreads), dim3(kTcfThreads), 0, s, a);
    return hipGetLastError();
}

// the checks both launches make of a window and its slices
static bool tcf_window_ok(int nblk, int slots, int ents, int stride, int n_live, int lag_first, int chunk, int slices)
{
    return nblk >= 1 && slots >= 1 && slots <= kTcfMaxOrigins && ents == slots + 1 && stride >= 1 && n_live >= 1 &&
           n_live <= slots && lag_first <= kTcfMaxLag && lag_first - (n_live - 1) * stride >= 1 && chunk >= 1 &&
           chunk <= kTcfMaxChunk && slices >= 1 && slices <= slots && (long long)slices * chunk >= n_live &&
           (long long)(slices - 1) * chunk < n_live;
}

hipError_t launch_tcf_terms(const TcfTermsArgs &a, hipStream_t s)
{
    if (!a.cur || !a.ring || !a.part || !a.flag || a.n_pad != (size_t)a.nblk * kTcfBlock || a.slot_first < 0 ||
        a.slot_first >= a.slots || !tcf_window_ok(a.nblk, a.slots, a.ents, a.stride, a.n_live, a.lag_first, a.chunk, a.slices))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(tcf_terms_kernel, dim3(a.nblk, a.slices), dim3(kTcfThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_tcf_fold(const TcfFoldArgs &a, hipStream_t s)
{
    if (!a.part || !a.flag || !a.sums || !a.range || a.max_lag < 1 || a.max_lag > kTcfMaxLag || a.lag_first > a.max_lag ||
        !tcf_window_ok(a.nblk, a.slots, a.ents, a.stride, a.n_live, a.lag_first, a.chunk, a.slices))
        return hipErrorInvalidValue;
    const int threads = 2 * (a.n_live + 1);
    hipLaunchKernelGGL(tcf_fold_kernel, dim3((threads + kTcfThreads - 1) / kTcfThreads), dim3(kTcfThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace ljmdt
