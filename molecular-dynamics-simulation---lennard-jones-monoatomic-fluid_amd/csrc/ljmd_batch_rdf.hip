// ljmd_batch_rdf.hip -- gfx950 kernel of the batch engine's g(r) accumulation (include/ljmd.h: ljmd_batch_rdf_*): the
// pair-distance histogram of the positions resident now, of every replica of a launch, one workgroup per replica.
//
// Per replica b, with its own n, L, rmax and dr = rmax / nbins, exactly what ljmd_rdf_histogram (rdf_histogram_kernel,
// ljmd_kernels.hip) computes for one snapshot of one system, through the same rdf_image and rdf_bin (ljmd_internal.h) --
// the reference's numpy arithmetic with its roundings
// (scripts/md_one_run_analysis.py:570-584):
//   d = x_j - x_i ; d -= L * rint(d / L)      (np.rint = half-to-even; a true division)
//   r = sqrt(dx*dx + dy*dy + dz*dz)           (unfused, correctly rounded sqrt)
//   if r < rmax: hist[b][int(r / dr)] += 2    (i < j pairs, weight 2)
// Compiled with -ffp-contract=off (csrc/Makefile).  The counts are integers, so they depend on no order: not on B, on
// the replica's slot, on the grouping into launches or on the streams.
//
// Shape: the batch kernel's (ljmd_batch.hip).  The replica's positions are loaded once into LDS (SoA, 3 NMAX doubles);
// a thread tid < T = batch_threads(n) owns particles tid, tid + T, ... (K of them); j is uniform across the wave, so
// every position read is a broadcast.  Every unordered pair is visited once (j > i): a wave starts j behind its first
// own particle.  The histogram lives in LDS (nbins 32-bit bins, ds_add_u32; one launch adds at most n (n - 1) <=
// 1.68e7 to a bin) and is added after a barrier into the replica's own row of the handle's 64-bit histogram with plain
// loads, adds and stores: the workgroup is the row's only writer, and launches on one stream follow one another.
#include "ljmd_batch.h"
#include "ljmd_internal.h"

namespace ljmdb {
namespace {

using ljmdk::rdf_bin;
using ljmdk::rdf_image;

template <int NMAX, int K>
__global__ __launch_bounds__(kBatchMaxThreads) void batch_rdf_kernel(BatchRdfArgs a)
{
    __shared__ double pos[3 * NMAX];
    extern __shared__ unsigned lhist[];     // [nbins]
    const BatchReplica &rp = a.rep[a.g0 + blockIdx.x];
    const int n = rp.n, T = rp.threads, tid = threadIdx.x, nbins = a.nbins;
    const double L = rp.L, invL = rp.invL;
    const size_t b = (size_t)rp.b;
    const BatchRdfReplica &rr = a.rdf[b];
    const double rmax = rr.rmax, dr = rr.dr, inv_dr = rr.inv_dr;
    const double *const R = a.r;
    const size_t plane = a.plane, base = rp.off;

    for (int i = tid; i < n; i += blockDim.x) {
        pos[i] = R[base + i];
        pos[NMAX + i] = R[plane + base + i];
        pos[2 * NMAX + i] = R[2 * plane + base + i];
    }
    for (int k = tid; k < nbins; k += blockDim.x) lhist[k] = 0u;
    __syncthreads();

    if (tid < T) {     // wave-uniform (T is a multiple of 64); the waves from T on own nothing
#pragma unroll 1
        for (int k = 0; k < K; ++k) {
            const int i = tid + k * T;
            const bool live = i < n;
            const double xi = live ? pos[i] : 0.0, yi = live ? pos[NMAX + i] : 0.0, zi = live ? pos[2 * NMAX + i] : 0.0;
            // the wave's first own particle of this pass: no j at or before it pairs with any of the wave's
            const int j0 = __builtin_amdgcn_readfirstlane((tid & ~63) + k * T) + 1;
            for (int j = j0; j < n; ++j) {
                double dx = pos[j] - xi, dy = pos[NMAX + j] - yi, dz = pos[2 * NMAX + j] - zi;
                dx = dx - L * rdf_image(dx, L, invL);
                dy = dy - L * rdf_image(dy, L, invL);
                dz = dz - L * rdf_image(dz, L, invL);
                const double r = __builtin_sqrt(dx * dx + dy * dy + dz * dz);
                if (live && j > i && r < rmax) {
                    const int bin = rdf_bin(r, dr, inv_dr);
                    if (bin < nbins) atomicAdd(&lhist[bin], 2u);
                }
            }
        }
    }
    __syncthreads();
    unsigned long long *const row = a.hist + b * (size_t)nbins;
    for (int k = tid; k < nbins; k += blockDim.x) {
        const unsigned c = lhist[k];
        if (c) row[k] = row[k] + (unsigned long long)c;
    }
}

}  // namespace

hipError_t launch_batch_rdf(const BatchRdfArgs &a, int n_max, int n_blocks, hipStream_t s)
{
    if (a.nbins < 1 || a.nbins > kBatchRdfMaxBins) return hipErrorInvalidValue;
    return dispatch_class(n_max, n_blocks, [&](auto nmax, auto k) {
        static_assert(3 * nmax() * sizeof(double) + kBatchRdfMaxBins * sizeof(unsigned) <= 160 * 1024, "LDS of one CU");
        hipLaunchKernelGGL((batch_rdf_kernel<nmax(), k()>), dim3(n_blocks), dim3(batch_threads(n_max)),
                           (size_t)a.nbins * sizeof(unsigned), s, a);
    });
}

}  // namespace ljmdb
