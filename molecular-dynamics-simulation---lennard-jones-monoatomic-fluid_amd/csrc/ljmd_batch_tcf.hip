// ljmd_batch_tcf.hip -- gfx950 kernel of the batch engine's MSD / VACF accumulation (include/ljmd.h: ljmd_batch_tcf_*):
// one snapshot of every replica of a launch against the origins stored in the ring, one workgroup per replica.
//
// Per replica, particle i, live origin t0 and lag l = s - t0 the reference's numpy expressions, unfused
// (scripts/md_one_run_analysis.py:404-489; compiled with -ffp-contract=off, csrc/Makefile):
//   MSD : d = ru(s) - ru(t0) per axis ; t = (dx*dx + dy*dy) + dz*dz
//   VACF: t = (vx(s)*vx(t0) + vy(s)*vy(t0)) + vz(s)*vz(t0)
// Every term enters an exact integer sum as Q(t) = RNE(t 2^64), |t| < 2^40 (else it enters as 0 and the replica's
// sticky range word is set).  Integer sums depend on no order: not on B, on the replica's slot, on the grouping into
// launches, on the streams, on the precision mode or on the order of the particles.
//
// Shape: the batch kernels' (ljmd_batch.hip), without a pair loop and without positions in LDS: the kernel streams.  A
// thread tid < T = batch_threads(n) owns particles tid, tid + T, ... (K of them) and keeps their current ru and v in
// registers (6 K doubles); per live origin it reads its own elements of the ring slot (coalesced) and forms the two
// terms.  Q(t) is an integer-valued double below 2^104, split exactly at 2^52 into two int64 limbs; a wave's 64 K <= 256
// terms sum to less than 2^60 per limb, so the limbs are reduced by integer shuffles, and lane 0 adds the wave's 128-bit
// total into the origin's LDS entry: two 64-bit integer LDS adds, the carry of the low word taken from the value the
// first add returns.  No barrier per origin.  After ONE barrier the workgroup adds its entries into its own rows of the
// 192-bit sums with plain loads, add192 and stores: it is the rows' only writer, and launches on one stream follow
// one another.  No global atomics, no floating-point atomics.  LDS: 32 bytes per live origin, one entry more for the
// lag-0 terms: at most 513 * 32 = 16416 bytes.
// Frame, current snapshot, ring walk, store of the snapshot and the closing addition into the rows are shared with
// batch_vanhove_kernel (ljmd_batch_origins_dev.h, BatchOriginArgs); tcf_origin and the one-barrier loop are this kernel's.
#include "ljmd_batch_origins_dev.h"
#include "ljmd_tcf_arith.h"

namespace ljmdb {
namespace {

using ljmdk::tcf_origin;

template <int NMAX, int K>
__global__ __launch_bounds__(kBatchMaxThreads) void batch_tcf_kernel(BatchTcfArgs a)
{
    extern __shared__ unsigned long long acc[];     // [n_live (+ 1)][2 kinds][2 words]
    const BatchOriginFrame f = batch_origin_frame(a, acc);
    const int n = f.n, T = f.T, tid = threadIdx.x;
    const size_t plane = a.plane;
    __syncthreads();

    bool bad = false;
    if (tid < T) {     // wave-uniform (T is a multiple of 64); the waves from T on own nothing
        const int lane = tid & 63;
        double cur[K][6];
        #pragma unroll
        for (int k = 0; k < K; ++k)
#pragma unroll
            for (int c = 0; c < 6; ++c) cur[k][c] = batch_origin_current(a, f, true, k, c);
        int slot = a.slot_first;
#pragma unroll 1
        for (int e = 0; e < f.n_live; ++e) {
            const double *const o = batch_origin_next<6>(a, f, slot);
            const auto org = [=](int k, int c) {
                const int i = tid + k * T;
                return i < n ? o[(size_t)c * plane + i] : 0.0;
            };
            tcf_origin(cur, org, f.lag0 && e == f.n_live - 1, lane, acc + 4 * e, acc + 4 * f.n_live, bad);
        }
        batch_origin_store(a, f, cur);
    }
    if (bad) a.range[f.b] = 1;
    __syncthreads();
    batch_origin_add_rows(a, f, acc);
}

}  // namespace

hipError_t launch_batch_tcf(const BatchTcfArgs &a, int n_max, int n_blocks, hipStream_t s)
{
    if (!batch_origin_window_ok(a, kBatchTcfMaxLag, kBatchTcfMaxOrigins)) return hipErrorInvalidValue;
    return dispatch_class(n_max, n_blocks, [&](auto nmax, auto k) {
        static_assert((kBatchTcfMaxOrigins + 1) * 32 <= 24 * 1024, "LDS budget of the accumulators");
        hipLaunchKernelGGL((batch_tcf_kernel<nmax(), k()>), dim3(n_blocks), dim3(batch_threads(n_max)),
                           (size_t)(a.n_live + 1) * 32, s, a);
    });
}

}  // namespace ljmdb
