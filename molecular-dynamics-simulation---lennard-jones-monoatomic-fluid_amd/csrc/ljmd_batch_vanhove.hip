// ljmd_batch_vanhove.hip -- gfx950 kernel of the batch engine's van Hove self-correlation G_s(r, tau) (include/ljmd.h:
// ljmd_batch_vanhove_*): one snapshot of every replica of a launch against the origins stored in the ring, one workgroup
// per replica.  Snapshots, origins and ring are those of the batch MSD / VACF accumulation (ljmd_batch_tcf.hip) with the
// unwrapped positions alone; per replica b, particle i, live origin t0 and lag l = s - t0, unfused (-ffp-contract=off):
//   d = ru(s) - ru(t0) per axis ; r2 = (dx*dx + dy*dy) + dz*dz   (the MSD term, bit for bit)
//   r4 = r2 * r2 ; r = sqrt(r2) ; bin = int(r / dr_b)             (rdf_bin)
// H[b][l][bin < nbins ? bin : nbins] += 1, S2[b][l] += Q(r2), S4[b][l] += Q(r4) with Q(t) = RNE(t 2^64)
// (ljmd_tcf_arith.h).  A particle whose r4 is not finite or >= 2^40 counts in the overflow column, enters both sums as 0
// and sets the replica's sticky range word; no float-to-int conversion sees such a value.  Counts and sums are integers:
// they depend on no order, so not on B, the replica's slot, the grouping into launches, the streams, the precision mode
// or the order of the particles.
//
// Shape: batch_tcf_kernel's.  A thread tid < T = batch_threads(n) owns particles tid, tid + T, ... (K of them) and keeps
// their current ru in registers (3 K doubles); per live origin it reads its own elements of the ring slot (coalesced),
// forms r2, r4 and the bin, increments the workgroup's 32-bit LDS histogram (i < n only: a padding lane would land in bin
// 0) and adds the limbs of Q(r2), Q(r4), summed over the wave by integer shuffles, into the origin's LDS entry.  After a
// barrier the non-zero bins are added into the replica's own row H[b][lag][.] with plain 64-bit loads, adds and stores
// -- the workgroup is the row's only writer, and launches on one stream follow one another -- and cleared; a second
// barrier precedes the next origin.  Both barriers are executed by EVERY thread of the workgroup: the waves from T on,
// which own nothing, walk the origin loop too (unlike batch_tcf_kernel, whose loop has no barrier and sits under
// tid < T).  The lag-0 row of the newest origin (when that is at lag 1) is one more pass of the same loop with the origin
// in the place of the snapshot.  At the end the workgroup adds its entries into its rows of the 192-bit sums as
// batch_tcf_kernel does, and the snapshot is stored into its ring slot when it is an origin.  No global atomics, no
// floating-point atomics, no spin-waits.  A 32-bit LDS bin holds at most n <= 4096 between two clears.
// LDS: 32 bytes per live origin, one entry more for the lag-0 terms, and 4 (nbins + 1) bytes of bins: at most
// 513 * 32 + 1025 * 4 = 20516 bytes.
// Frame, current snapshot, ring walk, store of the snapshot and the closing addition into the rows are shared with
// batch_tcf_kernel (ljmd_batch_origins_dev.h); the per-particle body, the bins and the two-barrier loop are this kernel's.
#include "ljmd_batch_origins_dev.h"
#include "ljmd_batch_vanhove.h"
#include "ljmd_tcf_arith.h"

namespace ljmdb {
namespace {

using namespace ljmdk;

template <int NMAX, int K>
__global__ __launch_bounds__(kBatchMaxThreads) void batch_vanhove_kernel(BatchVanhoveArgs a)
{
    extern __shared__ unsigned long long acc[];     // [n_live + 1][2 kinds][2 words], then the bins
    const BatchOriginFrame f = batch_origin_frame(a, acc);
    const int n = f.n, T = f.T, tid = threadIdx.x, lane = tid & 63;
    const size_t plane = a.plane;
    const int n_live = a.n_live, cols = a.nbins + 1, rows = a.max_lag + 1;
    unsigned *const lhist = reinterpret_cast<unsigned *>(acc + 4 * (n_live + 1));  // [nbins + 1]
    const double dr = a.dr[f.b], inv_dr = a.inv_dr[f.b];

    for (int k = tid; k < cols; k += blockDim.x) lhist[k] = 0u;
    __syncthreads();

    const bool own = tid < T;           // wave-uniform (T is a multiple of 64); the waves from T on own nothing
    double cur[K][3];
    #pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c) cur[k][c] = batch_origin_current(a, f, own, k, c);

    bool bad = false;
    int slot = a.slot_first;
#pragma unroll 1
    for (int e = 0; e < f.n_ent; ++e) { // uniform across the workgroup: every thread meets both barriers
        const bool zero = e == n_live;  // the lag-0 pass: the newest origin against itself
        if (zero) slot = slot == 0 ? a.slots - 1 : slot - 1;
        const double *const o = batch_origin_next<3>(a, f, slot);
        const int lag = zero ? 0 : a.lag_first - e * a.stride;
        if (own) {
            long long s_hi = 0, s_lo = 0, q_hi = 0, q_lo = 0;       // limbs of Q(r2) and Q(r4) of this origin
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int i = tid + k * T;
                double org[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) org[c] = i < n ? o[(size_t)c * plane + i] : 0.0;
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
                    if (r * inv_dr < (double)cols) bin = min(rdf_bin(r, dr, inv_dr), a.nbins);
                }
                if (i < n) atomicAdd(&lhist[bin], 1u);
            }
            s_hi = wave_sum_i64(s_hi);
            s_lo = wave_sum_i64(s_lo);
            q_hi = wave_sum_i64(q_hi);
            q_lo = wave_sum_i64(q_lo);
            if (lane == 0) {
                entry_add(acc + 4 * e, s_hi, s_lo);
                entry_add(acc + 4 * e + 2, q_hi, q_lo);
            }
        }
        __syncthreads();                            // the origin's histogram is complete
        if (lag >= 0 && lag < rows) {               // always, with the host's arguments
            unsigned long long *const hrow = a.hist + ((size_t)f.b * rows + lag) * cols;
            for (int k = tid; k < cols; k += blockDim.x) {
                const unsigned c = lhist[k];
                if (c) {
                    hrow[k] += (unsigned long long)c;
                    lhist[k] = 0u;
                }
            }
        }
        __syncthreads();                            // cleared before the next origin increments
    }
    if (own) batch_origin_store(a, f, cur);
    if (bad) a.range[f.b] = 1;
    // the entries are complete: the last entry_add lies before the loop's barriers
    batch_origin_add_rows(a, f, acc);
}

}  // namespace

hipError_t launch_batch_vanhove(const BatchVanhoveArgs &a, int n_max, int n_blocks, hipStream_t s)
{
    if (!a.state || !a.ring || !a.hist || !a.sums || !a.range || !a.dr || !a.inv_dr || !a.rep || a.g0 < 0 ||
        a.nbins < 1 || a.nbins > kBatchVanhoveMaxBins)
        return hipErrorInvalidValue;
    if (!batch_origin_window_ok(a, kBatchVanhoveMaxLag, kBatchVanhoveMaxOrigins)) return hipErrorInvalidValue;
    return dispatch_class(n_max, n_blocks, [&](auto nmax, auto k) {
        static_assert((kBatchVanhoveMaxOrigins + 1) * 32 + (kBatchVanhoveMaxBins + 1) * 4 <= 24 * 1024,
                      "LDS budget of the entries and the bins");
        hipLaunchKernelGGL((batch_vanhove_kernel<nmax(), k()>), dim3(n_blocks), dim3(batch_threads(n_max)),
                           (size_t)(a.n_live + 1) * 32 + (size_t)(a.nbins + 1) * 4, s, a);
    });
}

}  // namespace ljmdb
