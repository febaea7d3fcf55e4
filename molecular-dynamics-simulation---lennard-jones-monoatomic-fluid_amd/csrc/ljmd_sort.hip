// ljmd_sort.hip -- spatial re-ordering of the owned shard (performance only) and the ownership migration of multi-GPU runs.
//
// The shard is kept in k-d order (recursive median split, below): 64 consecutive slots (one tile = one wave) are a
// near-cubic box of exactly 64 particles.  Compact tiles are what lets the tile-pair test prove that whole 64 x 64 tile
// pairs lie outside the cutoff.  Correctness never depends on the order: bounding boxes are recomputed exactly from the
// actual coordinates before every force evaluation.  The (key, slot) radix sorts are stable and deterministic, so the
// summation order -- and hence every bit of the result -- is reproducible run to run.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include "ljmd_internal.h"
#include "ljmd_sort.h"

namespace ljmdk {

__global__ __launch_bounds__(kBlock) void gather_state_kernel(GatherStateArgs g)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= g.P) return;
    const int s = g.idx[i];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (g.src[q] == nullptr) continue;
#pragma unroll
        for (int k = 0; k < 3; ++k) g.dst[q][(size_t)k * g.P + i] = g.src[q][(size_t)k * g.P + s];
    }
    g.perm_out[i] = g.perm[s];
}

// ---- k-d ordering: recursive median split, exactly 64 particles per leaf ---------------
// Level l splits every current segment (a run of whole tiles) in two halves of whole tiles along
// axis l % 3: sorting each segment on that coordinate puts the lower half first.  After
// ceil(log2(#tiles)) levels every tile is a near-cubic box holding exactly 64 particles -- the
// most compact tiles a wave-sized group can have, which is what maximises the number of tile
// pairs the mask can prove to be outside the cutoff.
// key = (segment index << 24) | coordinate quantised to 24 bits: ONE ordinary radix sort per level
// orders every segment along the axis at once.  (A segmented sort of raw doubles gives the same
// order but is ~20x slower in rocPRIM for thousands of small segments.)

// the coordinate part of a key, for every kernel that builds one: scale = 2^kCoordBits / L (ljmd_sort.h)
__device__ __forceinline__ unsigned long long kd_quant(double coord, double scale)
{
    const double x = coord * scale;
    return (unsigned long long)fmin(fmax(x, 0.0), (double)((1u << kCoordBits) - 1));
}

__global__ __launch_bounds__(kBlock) void kd_keys_kernel(const double *coord, const int *idx, unsigned long long *keys,
                                                         const int *seg_offsets, int nseg, int S, double scale)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= S) return;
    int lo = 0, hi = nseg;                              // largest j with seg_offsets[j] <= i
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (seg_offsets[mid] <= i) lo = mid; else hi = mid;
    }
    keys[i] = ((unsigned long long)lo << kCoordBits) | kd_quant(coord[idx[i]], scale);
}

__global__ __launch_bounds__(kBlock) void iota_kernel(int *idx, int P)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i < P) idx[i] = i;
}

size_t kd_temp_bytes(int count)
{
    size_t bytes = 0;
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, (const unsigned long long *)nullptr,
                                             (unsigned long long *)nullptr, (const int *)nullptr, (int *)nullptr,
                                             count, 0, 64, nullptr);
    return bytes;
}

hipError_t launch_iota(int *idx, int P, hipStream_t s)
{
    hipLaunchKernelGGL(iota_kernel, dim3((P + kBlock - 1) / kBlock), dim3(kBlock), 0, s, idx, P);
    return hipGetLastError();
}

hipError_t kd_level(void *temp, size_t temp_bytes, const double *coord_axis, double L, unsigned long long *keys,
                    unsigned long long *keys_out, int *idx, int *idx_out, int S, int nseg, const int *seg_offsets,
                    hipStream_t s)
{
    hipLaunchKernelGGL(kd_keys_kernel, dim3((S + kBlock - 1) / kBlock), dim3(kBlock), 0, s, coord_axis, idx, keys,
                       seg_offsets, nseg, S, (double)(1u << kCoordBits) / L);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    int segbits = 1;
    while ((1 << segbits) < nseg) ++segbits;
    return hipcub::DeviceRadixSort::SortPairs(temp, temp_bytes, keys, keys_out, idx, idx_out, S, 0,
                                              kCoordBits + segbits, s);
}

// ---- the lower k-d levels in one launch -------------------------------------------------
// From the first level whose largest segment fits kKdFinishCap slots, one workgroup owns one segment of that level: the
// segments of every later level lie inside it, so it sorts its slice of the index array level after level in LDS and
// writes it back once.  A level is the same stable sort as kd_level's: by (segment, quantised coordinate), ties in their
// current order.  The current position is made part of the sort word, which makes the words distinct, so the order a
// bitonic network leaves is that stable order and the permutation equals the library sort's for every input.
// sort word: [63:56] segment of this level inside the slice (< 64), [55:32] kd_quant, [31:16] current position in the
// slice, [15:0] position the slot had when the kernel started (the index array's slice stays where it was loaded).
// 48 KB of LDS, 16 waves: one workgroup per CU, 64 of them at n = 262144 (0.17 ms for six levels).

// largest j in [0, n) with b[j] <= x; b ascending, b[0] <= x
__device__ __forceinline__ int last_at_most(const int *b, int n, int x)
{
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (b[mid] <= x) lo = mid; else hi = mid;
    }
    return lo;
}

// one compare-exchange of a bitonic network: x before y in the direction `up`
__device__ __forceinline__ void order_pair(unsigned long long &x, unsigned long long &y, bool up)
{
    if ((x > y) == up) {
        const unsigned long long t = x;
        x = y;
        y = t;
    }
}

__global__ __launch_bounds__(kKdFinishBlock) void kd_finish_kernel(KdFinishArgs a)
{
    constexpr int kMaxSub = kKdFinishCap / kTile;        // segments of a level inside one slice
    __shared__ unsigned long long s_word[kKdFinishCap];
    __shared__ int s_idx[kKdFinishCap];
    __shared__ int s_bound[kKdFinishMaxLevels][kMaxSub + 1];
    __shared__ int s_first[kKdFinishMaxLevels], s_last[kKdFinishMaxLevels];
    const int tid = threadIdx.x;
    const int lo = a.offsets[a.off[0] + blockIdx.x], len = a.offsets[a.off[0] + blockIdx.x + 1] - lo;
    if (len <= 0 || len > kKdFinishCap) return;          // (the host moves a level here only if every segment fits)
    int npad = kTile;
    while (npad < len) npad <<= 1;
    for (int p = tid; p < len; p += kKdFinishBlock) s_idx[p] = a.idx_in[lo + p];
    // every level's boundaries inside the slice, relative to lo, up front: the levels nest, so lo and lo + len are among
    // the boundaries of each (searched by all threads at once: a chain of dependent loads per level costs more)
    if (tid < kKdFinishMaxLevels) s_first[tid] = s_last[tid] = 0;
    __syncthreads();
    for (int l = 0; l < a.nlevels; ++l)
        for (int j = tid; j <= a.nseg[l]; j += kKdFinishBlock) {
            const int b = a.offsets[a.off[l] + j];
            if (b == lo) s_first[l] = j;
            if (b == lo + len) s_last[l] = j;
        }
    __syncthreads();
    for (int l = 0; l < a.nlevels; ++l) {
        const int nsub = min(s_last[l] - s_first[l], kMaxSub);
        if (tid <= nsub) s_bound[l][tid] = a.offsets[a.off[l] + s_first[l] + tid] - lo;
    }
    __syncthreads();
    for (int l = 0; l < a.nlevels; ++l) {
        const int nsub = min(s_last[l] - s_first[l], kMaxSub);
        const double *coord = a.pos + (size_t)a.axis[l] * a.P;
        for (int p = tid; p < npad; p += kKdFinishBlock) {
            unsigned long long w = ~0ull;                // padding: behind every slot of the slice
            if (p < len) {
                const unsigned home = l == 0 ? (unsigned)p : (unsigned)(s_word[p] & 0xffffu);
                const int sub = last_at_most(s_bound[l], nsub, p);
                w = ((unsigned long long)sub << 56) | (kd_quant(coord[s_idx[home]], a.scale) << 32) |
                    ((unsigned long long)p << 16) | home;
            }
            s_word[p] = w;
        }
        __syncthreads();
        for (int k = 2; k <= npad; k <<= 1) {
            int j = k >> 1;
            for (; j >= 2; j >>= 2) {                    // stages j and j / 2 in one pass over LDS: a thread holds the
                const int h = j >> 1;                    // four words whose positions differ in those two bits
                for (int t = tid; t < (npad >> 2); t += kKdFinishBlock) {
                    const int i = ((t & ~(h - 1)) << 2) | (t & (h - 1));
                    const bool up = (i & k) == 0;
                    unsigned long long w0 = s_word[i], w1 = s_word[i | h], w2 = s_word[i | j], w3 = s_word[i | j | h];
                    order_pair(w0, w2, up);
                    order_pair(w1, w3, up);
                    order_pair(w0, w1, up);
                    order_pair(w2, w3, up);
                    s_word[i] = w0;
                    s_word[i | h] = w1;
                    s_word[i | j] = w2;
                    s_word[i | j | h] = w3;
                }
                __syncthreads();
            }
            if (j == 1) {                                // an odd number of stages: the last one alone
                for (int t = tid; t < (npad >> 1); t += kKdFinishBlock) {
                    const int i = t << 1;
                    unsigned long long w0 = s_word[i], w1 = s_word[i | 1];
                    order_pair(w0, w1, (i & k) == 0);
                    s_word[i] = w0;
                    s_word[i | 1] = w1;
                }
                __syncthreads();
            }
        }
    }
    for (int p = tid; p < len; p += kKdFinishBlock) a.idx_out[lo + p] = s_idx[s_word[p] & 0xffffu];
}

hipError_t launch_kd_finish(const KdFinishArgs &a, hipStream_t s)
{
    if (a.nlevels < 1 || a.nlevels > kKdFinishMaxLevels) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kd_finish_kernel, dim3(a.nseg[0]), dim3(kKdFinishBlock), 0, s, a);
    return hipGetLastError();
}

// ---- ownership migration (multi-GPU): the particles of ALL ranks dealt out again by position -----------------------
// Every rank holds all n positions (exchange buffer [G][3][P], real particles in slots 0..S-1 of each block) and, after
// one all-gather, everybody's ru, v, a and particle ids (migration buffer [G][10][P]).  The deal is a k-d split of the
// n particles into G segments of exactly S = n / G: the same composite-key radix sort as above, over storage indices
// g * P + s, computed redundantly and identically (stable sort, same input bits) by every rank; rank r then takes
// segment r.  Blocks instead of slabs: a rank's surface, and with it the number of column tiles its rows meet at the
// cutoff, does not grow with G.
__global__ __launch_bounds__(kBlock) void iota_blocked_kernel(int *idx, int n, int S, int P)
{
    const int k = blockIdx.x * kBlock + threadIdx.x;
    if (k < n) idx[k] = (k / S) * P + k % S;
}

__global__ __launch_bounds__(kBlock) void kd_keys_blocked_kernel(const double *pos, int axis, int P, const int *idx,
                                                                 unsigned long long *keys, const int *seg_offsets, int nseg,
                                                                 int n, double scale)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    int lo = 0, hi = nseg;                              // largest j with seg_offsets[j] <= i
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (seg_offsets[mid] <= i) lo = mid; else hi = mid;
    }
    const int st = idx[i], g = st / P, sl = st - g * P;
    keys[i] = ((unsigned long long)lo << kCoordBits) | kd_quant(pos[(size_t)g * 3 * P + (size_t)axis * P + sl], scale);
}

// own block of the migration buffer: ru, v, a and the particle id of every slot (id < 0: padding)
__global__ __launch_bounds__(kBlock) void migrate_pack_kernel(const double *ru, const double *v, const double *a,
                                                              const int *perm, const int *gid0, double *block, int S, int P)
{
    const int s = blockIdx.x * kBlock + threadIdx.x;
    if (s >= P) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        block[(size_t)k * P + s] = ru[(size_t)k * P + s];
        block[(size_t)(3 + k) * P + s] = v[(size_t)k * P + s];
        block[(size_t)(6 + k) * P + s] = a[(size_t)k * P + s];
    }
    const int o = perm[s];
    block[(size_t)9 * P + s] = (s < S && o < S) ? (double)gid0[o] : -1.0;     // ids < 2^31: exact in a double
}

// the rank's new members, in the order of its segment of the deal: positions into a scratch block, ru, v, a and the ids
// into place (their sources are in the migration buffer); padding as after ljmd_set_state
__global__ __launch_bounds__(kBlock) void migrate_select_kernel(const double *pos_all, const double *mig_all, const int *mine,
                                                                double *new_pos, double *ru, double *v, double *a, int *gid0,
                                                                int S, int P)
{
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= P) return;
    if (j >= S) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            new_pos[(size_t)k * P + j] = __builtin_nan("");
            ru[(size_t)k * P + j] = __builtin_nan("");
            v[(size_t)k * P + j] = 0.0;
            a[(size_t)k * P + j] = 0.0;
        }
        gid0[j] = -1;
        return;
    }
    const int st = mine[j], g = st / P, sl = st - g * P;
    const double *pb = pos_all + (size_t)g * 3 * P + sl;
    const double *mb = mig_all + (size_t)g * 10 * P + sl;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        new_pos[(size_t)k * P + j] = pb[(size_t)k * P];
        ru[(size_t)k * P + j] = mb[(size_t)k * P];
        v[(size_t)k * P + j] = mb[(size_t)(3 + k) * P];
        a[(size_t)k * P + j] = mb[(size_t)(6 + k) * P];
    }
    gid0[j] = (int)mb[(size_t)9 * P];
}

__global__ __launch_bounds__(kBlock) void iota_offset_kernel(int *idx, int count, int P, int offset)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i < P) idx[i] = i < count ? offset + i : -1;
}

hipError_t launch_iota_blocked(int *idx, int n, int S, int P, hipStream_t s)
{
    hipLaunchKernelGGL(iota_blocked_kernel, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, idx, n, S, P);
    return hipGetLastError();
}

hipError_t launch_iota_offset(int *idx, int count, int P, int offset, hipStream_t s)
{
    hipLaunchKernelGGL(iota_offset_kernel, dim3((P + kBlock - 1) / kBlock), dim3(kBlock), 0, s, idx, count, P, offset);
    return hipGetLastError();
}

hipError_t kd_level_blocked(void *temp, size_t temp_bytes, const double *pos, int axis, int P, double L,
                            unsigned long long *keys, unsigned long long *keys_out, int *idx, int *idx_out, int n, int nseg,
                            const int *seg_offsets, hipStream_t s)
{
    hipLaunchKernelGGL(kd_keys_blocked_kernel, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, pos, axis, P, idx, keys,
                       seg_offsets, nseg, n, (double)(1u << kCoordBits) / L);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    int segbits = 1;
    while ((1 << segbits) < nseg) ++segbits;
    return hipcub::DeviceRadixSort::SortPairs(temp, temp_bytes, keys, keys_out, idx, idx_out, n, 0, kCoordBits + segbits, s);
}

hipError_t launch_migrate_pack(const double *ru, const double *v, const double *a, const int *perm, const int *gid0,
                               double *block, int S, int P, hipStream_t s)
{
    hipLaunchKernelGGL(migrate_pack_kernel, dim3((P + kBlock - 1) / kBlock), dim3(kBlock), 0, s, ru, v, a, perm, gid0, block,
                       S, P);
    return hipGetLastError();
}

hipError_t launch_migrate_select(const double *pos_all, const double *mig_all, const int *mine, double *new_pos, double *ru,
                                 double *v, double *a, int *gid0, int S, int P, hipStream_t s)
{
    hipLaunchKernelGGL(migrate_select_kernel, dim3((P + kBlock - 1) / kBlock), dim3(kBlock), 0, s, pos_all, mig_all, mine,
                       new_pos, ru, v, a, gid0, S, P);
    return hipGetLastError();
}

hipError_t launch_gather_state(const GatherStateArgs &g, hipStream_t s)
{
    hipLaunchKernelGGL(gather_state_kernel, dim3((g.P + kBlock - 1) / kBlock), dim3(kBlock), 0, s, g);
    return hipGetLastError();
}

}  // namespace ljmdk
