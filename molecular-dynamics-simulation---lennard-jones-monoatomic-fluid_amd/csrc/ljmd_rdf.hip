// ljmd_rdf.hip -- gfx950 kernels of the engine's resident g(r) accumulation (include/ljmd.h: ljmd_rdf_*): the
// pair-distance histogram of the positions in the exchange buffer, where they live, in the engine's tile order.
//
// Per pair exactly what ljmd_rdf_histogram (rdf_histogram_kernel, ljmd_kernels.hip) computes, through the same rdf_image
// and rdf_bin (ljmd_internal.h) -- the reference's numpy arithmetic with its roundings
// (scripts/md_one_run_analysis.py:570-584):
//   d = x_j - x_i ; d -= L * rint(d / L)      (np.rint = half-to-even; a true division)
//   r = sqrt(dx*dx + dy*dy + dz*dz)           (unfused, correctly rounded sqrt)
//   if r < rmax: hist[int(r / dr)] += 2       (i < j pairs, weight 2)
// Compiled with -ffp-contract=off (csrc/Makefile).  The counts are integers: they depend on no order, so not on the slot
// order, the tile walk, the slices of the grid or the number of ranks.
//
// rdf_boxes_kernel: exact bounding box of every 64-slot tile (one wave per tile, NaN padding ignored) into the
// feature's own buffer -- the engine's boxes (d_bbox) belong to its force evaluation and are left alone.
//
// rdf_pairs_kernel: one wave per row tile (lane = own particle, in registers), kRdfWaves waves per workgroup sharing one
// LDS histogram; the column particles are wave-uniform, fetched with scalar loads as pair_tiles_kernel does.  The walk
// and its weights are RdfPairArgs' (ljmd_rdf.h).  A wave tests 64 column tiles at a time, lane = column tile, with
// rdf_tile_gap2 and visits the survivors: rdf_walk_tiles (ljmd_rdf.h), the one copy of that loop.  Nothing here waits
// for another wave or workgroup.
#include "ljmd_rdf.h"
#include "ljmd_internal.h"

namespace ljmdr {
namespace {

using ljmdk::kTile;
using ljmdk::rdf_bin;
using ljmdk::rdf_image;

__device__ __forceinline__ double wave_min_all(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmin(v, __shfl_xor(v, off, 64));
    return v;
}

__device__ __forceinline__ double wave_max_all(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
    return v;
}

__global__ __launch_bounds__(kRdfWaves * kTile) void rdf_boxes_kernel(RdfBoxArgs a)
{
    const int lane = threadIdx.x & 63;
    const int t = blockIdx.x * kRdfWaves + (threadIdx.x >> 6);
    if (t >= a.T) return;
    const int g = t / a.TB, tl = t - g * a.TB;
    const double *b = a.pos + (size_t)g * 3 * a.P + (size_t)tl * kTile + lane;
    const double x = b[0], y = b[a.P], z = b[2 * (size_t)a.P];
    const double inf = __builtin_inf();
    // a padding slot (NaN) takes part in neither bound
    const double lx = wave_min_all(x == x ? x : inf), ly = wave_min_all(y == y ? y : inf), lz = wave_min_all(z == z ? z : inf);
    const double hx = wave_max_all(x == x ? x : -inf), hy = wave_max_all(y == y ? y : -inf), hz = wave_max_all(z == z ? z : -inf);
    if (lane == 0) {
        double *o = a.bbox + (size_t)t * kRdfBoxStride;
        o[0] = lx; o[1] = ly; o[2] = lz;
        o[3] = hx; o[4] = hy; o[5] = hz;
    }
}

// the 64 x 64 pairs of one (row tile, column tile).  MODE 0: all of them; 1: column slot > row slot (the diagonal tile of
// the unordered walk); 2: column slot != row slot (the own tile of the ordered walk)
template <int MODE>
__device__ __forceinline__ void tile_pairs(const RdfPairArgs &a, const double *bx, double xi, double yi, double zi, int lane,
                                           unsigned weight, unsigned *lhist)
{
    const double *by = bx + a.P, *bz = by + a.P;
    for (int j0 = 0; j0 < kTile; j0 += 8) {
        double xj[8], yj[8], zj[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) { xj[k] = bx[j0 + k]; yj[k] = by[j0 + k]; zj[k] = bz[j0 + k]; }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            double dx = xj[k] - xi, dy = yj[k] - yi, dz = zj[k] - zi;
            dx = dx - a.L * rdf_image(dx, a.L, a.invL);
            dy = dy - a.L * rdf_image(dy, a.L, a.invL);
            dz = dz - a.L * rdf_image(dz, a.L, a.invL);
            const double r2 = dx * dx + dy * dy + dz * dz;
            // Prefilter: r = sqrt(r2) correctly rounded and r < rmax give sqrt(r2) < rmax (were sqrt(r2) >= rmax, its
            // rounding could not fall below the representable rmax), so r2 < rmax^2 < rmax2_up: a pair that fails here
            // fails r < rmax as well, and one that passes is decided by r < rmax itself.  NaN (padding) fails both.
            bool in = r2 < a.rmax2_up;
            if (MODE == 1) in = in && (j0 + k > lane);
            if (MODE == 2) in = in && (j0 + k != lane);
            if (in) {
                const double r = __builtin_sqrt(r2);
                if (r < a.rmax) {
                    const int bin = rdf_bin(r, a.dr, a.inv_dr);
                    if (bin < a.nbins) atomicAdd(&lhist[bin], weight);
                }
            }
        }
    }
}

__global__ __launch_bounds__(kRdfWaves * kTile) void rdf_pairs_kernel(RdfPairArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned lhist[];     // [nbins]
    __shared__ unsigned long long wcount[2];
    for (int b = threadIdx.x; b < a.nbins; b += kRdfWaves * kTile) lhist[b] = 0u;
    if (threadIdx.x < 2) wcount[threadIdx.x] = 0ull;
    __syncthreads();

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int Il = blockIdx.x * kRdfWaves + wave;               // own row tile, wave-uniform
    if (Il < a.TB) {
        const int I = a.rank * a.TB + Il;
        const int row = Il * kTile + lane;
        const double *own = a.pos + (size_t)a.rank * 3 * a.P;
        const double xi = own[row], yi = own[a.P + row], zi = own[2 * (size_t)a.P + row];
        const bool unordered = a.G == 1;
        const unsigned weight = unordered ? 2u : 1u;
        const int u0 = blockIdx.y * a.chunk, u1 = min(u0 + a.chunk, a.U);
        unsigned visited = 0, considered = 0;
        rdf_walk_tiles(I, u0, u1, a.T, unordered, a.bbox, a.skip, a.L, a.rmax2_skin, visited, considered, [&](int Jb) {
            const int gj = unordered ? 0 : Jb / a.TB;
            const double *bx = a.pos + (size_t)gj * 3 * a.P + (size_t)(Jb - gj * a.TB) * kTile;
            if (Jb != I)
                tile_pairs<0>(a, bx, xi, yi, zi, lane, weight, lhist);
            else if (unordered)
                tile_pairs<1>(a, bx, xi, yi, zi, lane, weight, lhist);
            else
                tile_pairs<2>(a, bx, xi, yi, zi, lane, weight, lhist);
        });
        if (lane == 0) {
            atomicAdd(&wcount[0], (unsigned long long)visited);
            atomicAdd(&wcount[1], (unsigned long long)considered);
        }
    }
    __syncthreads();
    for (int b = threadIdx.x; b < a.nbins; b += kRdfWaves * kTile) {
        const unsigned c = lhist[b];
        if (c) atomicAdd(&a.hist[b], (unsigned long long)c);
    }
    if (threadIdx.x < 2 && wcount[threadIdx.x]) atomicAdd(&a.count[threadIdx.x], wcount[threadIdx.x]);
}

}  // namespace

hipError_t launch_rdf_boxes(const RdfBoxArgs &a, hipStream_t s)
{
    if (a.T < 1 || a.TB < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rdf_boxes_kernel, dim3((a.T + kRdfWaves - 1) / kRdfWaves), dim3(kRdfWaves * kTile), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_rdf_pairs(const RdfPairArgs &a, dim3 grid, hipStream_t s)
{
    // what the kernel's indexing and its 32-bit LDS bins rest on
    if (a.nbins < 1 || a.nbins > kRdfMaxBins || a.chunk < 1 || a.chunk > kRdfMaxChunk || a.U < 1 || a.TB < 1 ||
        a.T != a.G * a.TB || a.rank < 0 || a.rank >= a.G || (a.G == 1 ? a.U != a.T / 2 + 1 : a.U != a.T) ||
        (long long)grid.x * kRdfWaves < a.TB || (long long)grid.y * a.chunk < a.U ||
        rdf_lds_bound(a.chunk, a.G == 1 ? 2 : 1) > 0xffffffffull)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(rdf_pairs_kernel, grid, dim3(kRdfWaves * kTile), (size_t)a.nbins * sizeof(unsigned), s, a);
    return hipGetLastError();
}

}  // namespace ljmdr
