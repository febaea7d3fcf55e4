// ljmd_vanhove.hip -- gfx950 kernels of the van Hove self-correlation G_s(r, tau) of the system resident on a one-rank
// engine (include/ljmd.h: ljmd_vanhove_*; layout and argument blocks: ljmd_vanhove.h).  Snapshots, origins and ring are
// those of the MSD / VACF accumulation (ljmd_tcf.hip) with the unwrapped positions alone; per particle, origin and lag
//   d = ru(s) - ru(t0) per axis ; r2 = (dx*dx + dy*dy) + dz*dz   (the MSD term, bit for bit)
//   r4 = r2 * r2 ; r = sqrt(r2) ; bin = int(r / dr)               (-ffp-contract=off, csrc/Makefile; rdf_bin)
// H[lag][bin < nbins ? bin : nbins] += 1, S2[lag] += Q(r2), S4[lag] += Q(r4) with Q(t) = RNE(t 2^64) (ljmd_tcf_arith.h).
// A particle whose r4 is not finite or >= 2^40 counts in the overflow column, enters both sums as 0 and raises the
// range flag; no float-to-int conversion sees such a value.  Counts and sums are integers: they depend on no order, so
// not on the slot order, the grid or how the three kernels split the work.
//
// No pair loop: the path streams, 24 n_pad bytes per live origin.
//   1. vanhove_gather_kernel  slot order -> particle-id order through the DEVICE's permutation; it also stores the
//                             snapshot into its ring slot when it becomes an origin.
//   2. vanhove_terms_kernel   grid (particle blocks, origin slices).  A thread keeps the current ru of its kVhK
//                             particles (ids block * 1024 + tid + k 256: coalesced) in registers and, per live origin of
//                             its slice, loads its own elements of the ring slot, forms r2, r4 and the bin, increments
//                             the workgroup's 32-bit LDS histogram (ids < n only: padding would land in bin 0) and adds
//                             the limbs of Q(r2), Q(r4), summed over the wave by integer shuffles, into the origin's LDS
//                             entry.  After a barrier the non-zero bins go to H[lag][.] by 64-bit integer atomicAdd and
//                             are cleared for the next origin.  The lag-0 row of the newest origin (when that is at
//                             lag 1) is one more pass of the same loop with the origin in the place of the snapshot.
//                             At the end the workgroup writes its entries by plain stores into its own rows of `part`.
//   3. vanhove_fold_kernel    one thread per (entry, kind): adds the entry's partials over all particle blocks into
//                             sums[kind][lag] (the row's only writer) and ORs the workgroups' range flags.
// The only global atomics are the integer adds into H; no floating-point atomics, no spin-waits, no dependency between
// workgroups inside a launch.  A 32-bit LDS bin holds at most kVhBlock = 1024 between two clears.
#include "ljmd_vanhove.h"

#include "ljmd_internal.h"
#include "ljmd_tcf_arith.h"

namespace ljmdv {
namespace {

using ljmdk::add192;
using ljmdk::entry_add;
using ljmdk::fixed_out_of_range;
using ljmdk::rdf_bin;
using ljmdk::tcf_add;
using ljmdk::wave_sum_i64;

__global__ __launch_bounds__(kVhThreads) void vanhove_gather_kernel(VhGatherArgs a)
{
    const int s = blockIdx.x * kVhThreads + threadIdx.x;
    if (s >= a.P) return;
    const int id = a.perm[s];
    if (id < 0 || id >= a.n) return;                // a padding slot
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double x = a.ru[(size_t)c * a.P + s];
        a.cur[(size_t)c * a.n_pad + id] = x;
        if (a.store) a.store[(size_t)c * a.n_pad + id] = x;
    }
}

__global__ __launch_bounds__(kVhThreads) void vanhove_terms_kernel(VhTermsArgs a)
{
    __shared__ unsigned long long acc[(kVhMaxChunk + 1) * 4];      // [origins of the slice (+ 1)][2 kinds][2 words]
    __shared__ unsigned lhist[kVhMaxBins + 1];                     // [nbins + 1]
    const int tid = threadIdx.x, lane = tid & 63;
    const int blk = blockIdx.x, slice = blockIdx.y;
    const int n_live = a.n_live, cols = a.nbins + 1;
    const int e0 = slice * a.chunk, e1 = min(n_live, e0 + a.chunk), n_loc = e1 - e0;
    // the newest origin is at lag 1 and belongs to this slice: its lag-0 terms go to the entry behind the slice's
    const bool lag0 = e1 == n_live && a.lag_first - (n_live - 1) * a.stride == 1;
    const int n_ent = n_loc + (lag0 ? 1 : 0);

    for (int k = tid; k < 4 * n_ent; k += kVhThreads) acc[k] = 0ull;
    for (int b = tid; b < cols; b += kVhThreads) lhist[b] = 0u;
    __syncthreads();

    const size_t np = a.n_pad, i0 = (size_t)blk * kVhBlock + tid;
    double cur[kVhK][3];
#pragma unroll
    for (int k = 0; k < kVhK; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c) cur[k][c] = a.cur[(size_t)c * np + i0 + (size_t)k * kVhThreads];

    bool bad = false;
    int slot = (a.slot_first + e0) % a.slots;
#pragma unroll 1
    for (int e = 0; e < n_ent; ++e) {
        const bool zero = e == n_loc;               // the lag-0 pass: the newest origin against itself (uniform)
        if (zero) slot = slot == 0 ? a.slots - 1 : slot - 1;
        const double *const o = a.ring + (size_t)slot * 3 * np + i0;
        slot = slot + 1 == a.slots ? 0 : slot + 1;
        const int lag = zero ? 0 : a.lag_first - (e0 + e) * a.stride;
        long long s_hi = 0, s_lo = 0, q_hi = 0, q_lo = 0;       // limbs of Q(r2) and Q(r4) of this origin
#pragma unroll
        for (int k = 0; k < kVhK; ++k) {
            double org[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) org[c] = o[(size_t)c * np + (size_t)k * kVhThreads];
            const double dx = (zero ? org[0] : cur[k][0]) - org[0], dy = (zero ? org[1] : cur[k][1]) - org[1],
                         dz = (zero ? org[2] : cur[k][2]) - org[2];
            const double r2 = (dx * dx + dy * dy) + dz * dz;
            const double r4 = r2 * r2;
            const bool oob = fixed_out_of_range(r4);             // true as well when r2 is not finite
            bad = bad || oob;
            tcf_add(s_hi, s_lo, oob ? 0.0 : r2, bad);
            tcf_add(q_hi, q_lo, oob ? 0.0 : r4, bad);
            int bin = a.nbins;
            if (!oob) {                                          // r2 < 2^20: r < 1024
                const double r = __builtin_sqrt(r2);
                // the product is within 2 ulp of r / dr: at nbins + 1 or beyond (or NaN) the quotient is >= nbins
                if (r * a.inv_dr < (double)cols) bin = min(rdf_bin(r, a.dr, a.inv_dr), a.nbins);
            }
            if (i0 + (size_t)k * kVhThreads < (size_t)a.n) atomicAdd(&lhist[bin], 1u);
        }
        s_hi = wave_sum_i64(s_hi);
        s_lo = wave_sum_i64(s_lo);
        q_hi = wave_sum_i64(q_hi);
        q_lo = wave_sum_i64(q_lo);
        if (lane == 0) {
            entry_add(acc + 4 * e, s_hi, s_lo);
            entry_add(acc + 4 * e + 2, q_hi, q_lo);
        }
        __syncthreads();                            // the origin's histogram is complete
        unsigned long long *const hrow = a.hist + (size_t)lag * cols;
        for (int b = tid; b < cols; b += kVhThreads) {
            const unsigned c = lhist[b];
            if (c) {
                atomicAdd(&hrow[b], (unsigned long long)c);
                lhist[b] = 0u;
            }
        }
        __syncthreads();                            // cleared before the next origin increments
    }
    const int any_bad = __syncthreads_or(bad ? 1 : 0);          // the entries are complete behind it

    // entries e0 .. e0 + n_ent - 1 of this block's row: the lag-0 entry of the last slice is entry n_live
    unsigned long long *const row = a.part + ((size_t)blk * a.ents + e0) * 4;
    for (int k = tid; k < 4 * n_ent; k += kVhThreads) row[k] = acc[k];
    if (tid == 0) a.flag[(size_t)blk * a.slots + slice] = any_bad;
}

__global__ __launch_bounds__(kVhThreads) void vanhove_fold_kernel(VhFoldArgs a)
{
    const int k = blockIdx.x * kVhThreads + threadIdx.x;
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

// the checks both launches make of a window and its slices
bool window_ok(int nblk, int slots, int ents, int stride, int max_lag, int n_live, int lag_first, int chunk, int slices)
{
    return nblk >= 1 && slots >= 1 && slots <= kVhMaxOrigins && ents == slots + 1 && stride >= 1 && max_lag >= 1 &&
           max_lag <= kVhMaxLag && n_live >= 1 && n_live <= slots && lag_first <= max_lag &&
           lag_first - (n_live - 1) * stride >= 1 && chunk >= 1 && chunk <= kVhMaxChunk && slices >= 1 && slices <= slots &&
           (long long)slices * chunk >= n_live && (long long)(slices - 1) * chunk < n_live;
}

}  // namespace

hipError_t launch_vanhove_gather(const VhGatherArgs &a, hipStream_t s)
{
    if (!a.ru || !a.perm || !a.cur || a.n < 1 || a.P < a.n || a.n_pad < (size_t)a.n || a.n_pad % kVhBlock != 0)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(vanhove_gather_kernel, dim3((a.P + kVhThreads - 1) / kVhThreads), dim3(kVhThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_vanhove_terms(const VhTermsArgs &a, hipStream_t s)
{
    if (!a.cur || !a.ring || !a.hist || !a.part || !a.flag || a.n_pad != (size_t)a.nblk * kVhBlock || a.n < 1 ||
        (size_t)a.n > a.n_pad || a.n_pad - (size_t)a.n >= (size_t)kVhBlock || a.nbins < 1 || a.nbins > kVhMaxBins ||
        !(a.dr > 0.0) || !(a.inv_dr > 0.0) || a.slot_first < 0 || a.slot_first >= a.slots ||
        !window_ok(a.nblk, a.slots, a.ents, a.stride, a.max_lag, a.n_live, a.lag_first, a.chunk, a.slices))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(vanhove_terms_kernel, dim3(a.nblk, a.slices), dim3(kVhThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_vanhove_fold(const VhFoldArgs &a, hipStream_t s)
{
    if (!a.part || !a.flag || !a.sums || !a.range ||
        !window_ok(a.nblk, a.slots, a.ents, a.stride, a.max_lag, a.n_live, a.lag_first, a.chunk, a.slices))
        return hipErrorInvalidValue;
    const int threads = 2 * (a.n_live + 1);
    hipLaunchKernelGGL(vanhove_fold_kernel, dim3((threads + kVhThreads - 1) / kVhThreads), dim3(kVhThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace ljmdv
