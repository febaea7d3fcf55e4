// ljmd_vanhove.hip -- gfx950 kernels of the van Hove self-correlation G_s(r, tau) of the system resident on a one-rank
// engine (include/ljmd.h: ljmd_vanhove_*; layout and argument blocks: ljmd_origins.h, ljmd_vanhove.h).  Snapshots,
// origins and ring are those of the MSD / VACF accumulation (ljmd_tcf.hip) with the unwrapped positions alone; per
// particle, origin and lag
//   d = ru(s) - ru(t0) per axis ; r2 = (dx*dx + dy*dy) + dz*dz   (the MSD term, bit for bit)
//   r4 = r2 * r2 ; r = sqrt(r2) ; bin = int(r / dr)               (-ffp-contract=off, csrc/Makefile; rdf_bin)
// H[lag][bin < nbins ? bin : nbins] += 1, S2[lag] += Q(r2), S4[lag] += Q(r4) with Q(t) = RNE(t 2^64) (ljmd_tcf_arith.h).
// A particle whose r4 is not finite or >= 2^40 counts in the overflow column, enters both sums as 0 and raises the
// range flag; no float-to-int conversion sees such a value.  Counts and sums are integers: they depend on no order, so
// not on the slot order, the grid or how the three kernels split the work.
//
// No pair loop: the path streams, 24 n_pad bytes per live origin.
//   1. origin_gather_kernel<3>  slot order -> particle-id order (ljmd_origins_dev.h).
//   2. vanhove_terms_kernel   grid (particle blocks, origin slices), its frame ljmd_origins_dev.h's.  A thread keeps the
//                             current ru of its kVhK particles in registers and, per live origin of its slice, loads its
//                             own elements of the ring slot, forms r2, r4 and the bin, increments the workgroup's 32-bit
//                             LDS histogram (ids < n only: padding would land in bin 0) and adds the limbs of Q(r2),
//                             Q(r4), summed over the wave by integer shuffles, into the origin's LDS entry.  After a
//                             barrier the non-zero bins go to H[lag][.] by 64-bit integer atomicAdd and are cleared for
//                             the next origin.  The lag-0 row of the newest origin (when that is at lag 1) is one more
//                             pass of the same loop with the origin in the place of the snapshot.  At the end the
//                             workgroup writes its entries by plain stores into its own rows of `part`.
//   3. origin_fold_kernel     the entries' partials over all particle blocks into sums[kind][lag] (ljmd_origins_dev.h).
// The only global atomics are the integer adds into H; no floating-point atomics, no spin-waits, no dependency between
// workgroups inside a launch.  A 32-bit LDS bin holds at most kVhBlock = 1024 between two clears.
#include "ljmd_vanhove.h"

#include "ljmd_origins_dev.h"
#include "ljmd_tcf_arith.h"

namespace ljmdv {
namespace {

using namespace ljmdk;

__global__ __launch_bounds__(kVhThreads) void vanhove_terms_kernel(VhTermsArgs a)
{
    __shared__ unsigned long long acc[(kVhMaxChunk + 1) * 4];      // [origins of the slice (+ 1)][2 kinds][2 words]
    __shared__ unsigned lhist[kVhMaxBins + 1];                     // [nbins + 1]
    const int tid = threadIdx.x, lane = tid & 63;
    const int cols = a.nbins + 1;
    const OriginSlice s = origin_slice(a);
    origin_zero_entries(acc, s);
    for (int b = tid; b < cols; b += kVhThreads) lhist[b] = 0u;
    __syncthreads();

    const size_t np = a.n_pad, i0 = origin_first_id();
    double cur[kVhK][3];
    origin_load_current(a, cur);

    bool bad = false;
    int slot = origin_first_slot(a, s);
#pragma unroll 1
    for (int e = 0; e < s.n_ent; ++e) {
        const bool zero = e == s.n_loc;             // the lag-0 pass: the newest origin against itself (uniform)
        if (zero) slot = slot == 0 ? a.slots - 1 : slot - 1;
        const double *const o = origin_next<3>(a, slot);
        const int lag = zero ? 0 : a.lag_first - (s.e0 + e) * a.stride;
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
    origin_write_rows(a, s, acc, bad);
}

}  // namespace

hipError_t launch_vanhove_gather(const VhGatherArgs &a, hipStream_t s) { return launch_origin_gather<3>(a, s); }

hipError_t launch_vanhove_terms(const VhTermsArgs &a, hipStream_t s)
{
    if (!a.cur || !a.ring || !a.hist || !a.part || !a.flag || a.n_pad != (size_t)a.nblk * kVhBlock || a.n < 1 ||
        (size_t)a.n > a.n_pad || a.n_pad - (size_t)a.n >= (size_t)kVhBlock || a.nbins < 1 || a.nbins > kVhMaxBins ||
        !(a.dr > 0.0) || !(a.inv_dr > 0.0) || a.slot_first < 0 || a.slot_first >= a.slots ||
        !origin_window_ok(a.nblk, a.slots, a.ents, a.stride, a.max_lag, a.n_live, a.lag_first, a.chunk, a.slices))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(vanhove_terms_kernel, dim3(a.nblk, a.slices), dim3(kVhThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_vanhove_fold(const VhFoldArgs &a, hipStream_t s) { return launch_origin_fold(a, s); }

}  // namespace ljmdv
