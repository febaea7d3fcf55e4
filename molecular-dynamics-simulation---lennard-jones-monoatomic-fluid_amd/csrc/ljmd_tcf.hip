// ljmd_tcf.hip -- gfx950 kernels of the MSD / VACF accumulation of the system resident on a one-rank engine
// (include/ljmd.h: ljmd_tcf_*; layout and argument blocks: ljmd_origins.h, ljmd_tcf.h).  The definition is the batch
// engine's (ljmd_batch_tcf.hip) with B = 1, and the arithmetic of one origin is the same code (ljmd_tcf_arith.h):
//   MSD : d = ru(s) - ru(t0) per axis ; t = (dx*dx + dy*dy) + dz*dz
//   VACF: t = (vx(s)*vx(t0) + vy(s)*vy(t0)) + vz(s)*vz(t0)            (-ffp-contract=off, csrc/Makefile)
// each entering an exact integer sum as Q(t) = RNE(t 2^64).  Integer sums depend on no order, so the result does not
// depend on the slot order, on the grid or on how the three kernels split the work.
//
// No pair loop: the path streams, its bound is HBM bandwidth -- 48 n_pad bytes per live origin.
//   1. origin_gather_kernel<6>  slot order -> particle-id order (ljmd_origins_dev.h): 48 n bytes.
//   2. tcf_terms_kernel   grid (particle blocks, origin slices), its frame ljmd_origins_dev.h's.  A thread keeps the
//                         current six values of its kTcfK particles in registers and, per live origin of its slice,
//                         loads its own elements of the ring slot and forms the two terms (and the lag-0 terms of the
//                         newest origin when that is at lag 1).  Limbs are summed over the wave by integer shuffles,
//                         lane 0 adds the wave's 128-bit total into the origin's LDS entry; after ONE barrier the
//                         workgroup writes its entries with plain stores into its own rows of `part`.
//   3. origin_fold_kernel the entries' partials over all particle blocks into sums[kind][lag] (ljmd_origins_dev.h).
// No global atomics, no floating-point atomics, no spin-waits, no dependency between workgroups inside a launch.
#include "ljmd_tcf.h"

#include "ljmd_origins_dev.h"
#include "ljmd_tcf_arith.h"

namespace ljmdt {
namespace {

using namespace ljmdk;

__global__ __launch_bounds__(kTcfThreads) void tcf_terms_kernel(TcfTermsArgs a)
{
    __shared__ unsigned long long acc[(kTcfMaxChunk + 1) * 4];     // [origins of the slice (+ 1)][2 kinds][2 words]
    const OriginSlice s = origin_slice(a);
    origin_zero_entries(acc, s);
    __syncthreads();

    double cur[kTcfK][6];
    origin_load_current(a, cur);

    bool bad = false;
    int slot = origin_first_slot(a, s);
#pragma unroll 1
    for (int e = 0; e < s.n_loc; ++e) {
        const double *const o = origin_next<6>(a, slot);
        const size_t np = a.n_pad;
        tcf_origin(cur, [=](int k, int c) { return o[(size_t)c * np + (size_t)k * kTcfThreads]; },
                   s.lag0 && e == s.n_loc - 1, threadIdx.x & 63, acc + 4 * e, acc + 4 * s.n_loc, bad);
    }
    origin_write_rows(a, s, acc, bad);
}

}  // namespace

hipError_t launch_tcf_gather(const TcfGatherArgs &a, hipStream_t s) { return launch_origin_gather<6>(a, s); }

hipError_t launch_tcf_terms(const TcfTermsArgs &a, hipStream_t s)
{
    // the block carries no max_lag: the window is checked against the largest one
    if (!a.cur || !a.ring || !a.part || !a.flag || a.n_pad != (size_t)a.nblk * kTcfBlock || a.slot_first < 0 ||
        a.slot_first >= a.slots ||
        !origin_window_ok(a.nblk, a.slots, a.ents, a.stride, kTcfMaxLag, a.n_live, a.lag_first, a.chunk, a.slices))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(tcf_terms_kernel, dim3(a.nblk, a.slices), dim3(kTcfThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_tcf_fold(const TcfFoldArgs &a, hipStream_t s) { return launch_origin_fold(a, s); }

}  // namespace ljmdt
