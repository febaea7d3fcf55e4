// ljmd_internal.h -- argument blocks shared by the kernels and the C-ABI host code, and (last section) the device
// arithmetic shared by the kernel files.
//
// HBM layout (all fp64, structure of arrays):
//   n      total particles, G ranks, S = n / G particles per rank ("shard"),
//   P      axis stride = S rounded up to a multiple of kBlock (256); slots S..P-1 of every
//          axis array are padding: position = NaN (never passes r^2 < rc^2), v = a = 0.
//   pos    exchange buffer [G][3][P]: block g = x[P] y[P] z[P] of rank g's particles.
//   ru,v,a [3][P] of the owned shard.
//   tiles  64 consecutive slots; TB = P / 64 tiles per rank block, T = G * TB tiles.
#ifndef LJMD_INTERNAL_H
#define LJMD_INTERNAL_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ljmdk {

constexpr int kBlock = 256;                 // threads per workgroup = 4 wave64
constexpr int kWavesPerBlock = kBlock / 64;
constexpr int kTile = 64;                   // particles per tile = one wave
#ifndef LJMD_ROW_TILES
#define LJMD_ROW_TILES 4
#endif
constexpr int kRowTiles = LJMD_ROW_TILES;   // tiles per Newton-3 row group (particles per lane)
constexpr unsigned kAllRows = (1u << kRowTiles) - 1u;
constexpr int kSlotAlign = (kRowTiles * 64 > 256) ? kRowTiles * 64 : 256;   // P is a multiple of this
constexpr int kPartialStride = 8;           // doubles per per-rank per-step partial record
constexpr int kFoldBlocks = 128;             // pre-reduction blocks of the scalar partials (large grids)
constexpr int kDirectFoldMax = 20480;        // workgroup partials up to which ONE block folds the step record (finalize_body) in every launch form
constexpr int kBoxStride = 8;               // doubles per tile bounding box (lo xyz, hi xyz, 2 pad)

struct PairArgs {
    const double *pos;      // exchange buffer [G][3][P]
    double *slab;           // [nslab][3][P] raw partial accelerations of the owned rows
    double *wg_part;        // [n workgroups][2] = s12, s6
    const uint64_t *mask;   // [TB][W] bit (J) of row I set = tile pair must be evaluated
    const double *bbox;     // tile kernel with inline_mask: the tile boxes [T][kBoxStride]
    int inline_mask;        // tile kernel, small single-rank systems: the waves work their mask words out themselves
                            // (tile_mask_kernel's test; `mask` unused) and the step saves a launch
    double rc2_skin;        // rc^2 (1 + 1e-10) of that test
    int n;                  // total particles
    int S;                  // real particles per rank
    int P;                  // padded axis stride
    int G;                  // ranks
    int rank;
    int TB;                 // tiles per rank block
    int T;                  // tiles in total
    int W;                  // 64-bit mask words per row = ceil(T / 64)
    int chunk;              // generic kernel: j slots per grid.y slice; tile kernel: column tiles per slice
    double L, invL, rc2;
};

// Newton-3 pair kernel (ljmd_kernels.hip: pair_n3_kernel).  Row group = kRowTiles (4) consecutive
// tiles = 256 slots held by ONE wave, 4 particles per lane.  NG = T / 4 groups.  A row group A
// owns the column groups B with cyclic offset d = (B - A) mod NG in [0, Dmax] (ties broken by
// index), so every unordered pair of particles is evaluated exactly once on the whole machine.
struct N3Args {
    const double *pos;      // exchange buffer
    const uint64_t *mask;   // [TB rows][W] tile-pair mask of the owned row tiles
    const double *bbox;     // [T][kBoxStride] exact tile bounding boxes (fp32 far kernel: image classification)
    const unsigned *desc;   // [NGo][T] pass descriptors of tile_class_kernel (row-tile mask bits, loop variant, images)
    const float *desc2;     // [NGo][T][8] cluster passes: direction n (3), thresholds of the RT row tiles (4), pad; or NULL
    double *slab_i;         // [nchunk][3][P] partial accelerations of the owned rows (row side)
    double *slab_j;         // [T][CS][3][64] column-side partial accelerations: one block per (column tile, workgroup of WG
                            // consecutive row groups); the CS blocks of a column tile lie together, so that the reduction
                            // streams them.  Block j of column tile c: by_group ? the workgroup's index : e / WG, with e =
                            // the column group's offset from the workgroup's first row group (single rank, WG | NG: one
                            // workgroup per value, CS = (Dmax + WG - 1) / WG + 1)
    unsigned char *flag_j;  // [T][CS] 1 = slab_j block written this step
    double *wg_part;        // [n workgroups][2]
    int S, P, G, rank, TB, T, W;   // S = real particles per rank (slots S..P-1 are padding)
    int NG, NGo, Dmax;      // row groups in total / owned by this rank (NGo = TB / RT, NG = G * NGo)
    int CS, by_group;       // slab_j layout (above)
    int RT;                 // tiles per row group: 4 for large systems, 1 or 2 to give small ones enough work items
    int dchunk;             // fp32 far kernel: offsets d per grid.y slice
    int by0;                // pair_n3_kernel: slice of this launch's blockIdx.y == 0.  0 unless the step runs the slices in two
                            // launches (LaunchPlan::split_s1): the work item of a slice does not depend on which launch runs it
    int uchunk;             // pair_n3_kernel: UNITS per grid.y slice.  Unit u of a row group = e * RT + l: offset e, column tile l of
                            // the group there (one pass); = dchunk * RT unless the system is cut finer
    int energy;             // 0: forces only -- the energy sums are not accumulated and the workgroup partials are NaN
    int xcd_remap;          // C > 0: XCD-aware mapping, chunks of C consecutive row groups per XCD (gridDim.x % (8 C) == 0)
    int inline_class;       // RT <= 2, one wave per workgroup: the waves compute their pass descriptors themselves (desc unused)
    int both_ties;          // one wave per workgroup, one rank: the tie d = NG / 2 (NG even) is worked from both sides, the
                            // steps 0 .. 31 by the lower row group and 1 .. 32 by the upper one (ljmd_kernels.hip: tile_of)
    double L, invL, rc2;
    double rc2_skin;        // rc^2 (1 + 1e-10) of the tile-pair test (GeometryArgs::rc2_skin), for inline_class
};

struct IntegrateArgs {
    double *r;              // own block of the exchange buffer, axis stride = P
    double *ru, *v, *a;     // [3][P]
    const double *fsum;     // [3][P] raw (prefactor-free) total accelerations of the owned rows
    double *ke_part;        // [n blocks][3]
    int rows;               // = P (padding included: it integrates to NaN / 0 harmlessly)
    int P;
    double L, invL, dt, dt_half, dt_sq_half;
    double *bbox;           // drift kernel, single rank: also emit the tile bounding boxes [P / 64][kBoxStride] (else NULL)
    double *pos_tc;         // ... and, on the Newton-3 path, the tile-coherent copy of the new positions [3][P] (else NULL)
    int RT;                 // tiles per Newton-3 row group (the frame of pos_tc is per group)
    unsigned *ticket;       // kick kernel with the finalize folded in: blocks-done counter (else NULL)
};

// Deterministic reduction of the pair kernels' partial-acceleration slabs into fpart.
// Gather kernels / single rank: fpart = [1][3][P] (own rows).  Newton-3 on G > 1 ranks:
// fpart = [G][3][P], block g = this rank's contributions to rank g's particles (own block:
// row side + column side, remote blocks: column side only); an RCCL reduce-scatter then sums
// block g over the ranks into rank g's fsum.
struct ReduceArgs {
    const double *slab;     // row side [nslab][3][P]
    const double *slab_j;   // column side (Newton-3) or NULL
    const unsigned char *flag_j;
    const float *slab_j2;   // second column-side set (fp32 far pass of the mixed-precision mode: [T][CS2] blocks of floats) or NULL
    const unsigned char *flag_j2;
    double *fpart;
    int nslab, P, G, rank, TB;
    int CS, CS2;            // blocks per column tile of slab_j / slab_j2 (N3Args::slab_j)
    int RT;                 // tiles per Newton-3 row group of this engine (1, 2 or 4)
    // two-phase form (reduce_forces_split_kernel; one rank): phase 1 sums the row-side slices c < c_split and the blocks
    // j < j_split of every column tile and leaves the four waves' partial sums in `partial`; phase 2 continues from them
    double *partial;        // [TB][4][3][64], or NULL
    int c_split, j_split;
};

struct FinalizeArgs {
    const double *wg_part;
    const double *ke_part;
    const double *ke_tile;  // NULL, or [T][3] per-tile sums of v^2 (tile_tail_kernel) to be combined per 256-slot block
    double *ring;           // [ring_cap][kPartialStride]
    unsigned *ring_pos;     // device counter, bumped once per finalize
    int n_wg, n_ke;
    unsigned ring_cap;
    double pair_scale;      // 0.5 when every unordered pair was visited twice (gather kernels), 1 for Newton-3
};

struct GeometryArgs {
    const double *pos;      // exchange buffer
    double *bbox;           // [T][kBoxStride]
    double *pos_tc;         // Newton-3 path: tile-coherent copy of pos, same layout (else NULL): every tile's particles in the
                            // periodic image nearest to the tile's first particle; bbox then bounds THOSE coordinates
    uint64_t *mask;         // [TB][W]
    uint64_t *mask_far;     // mixed precision only (else NULL): [TB][W] tile pairs evaluated in fp32;
                            // `mask` then holds only the NEAR pairs (box distance <= r_split, or same row group)
    int P, G, rank, TB, T, W;
    int RT;                 // tiles per Newton-3 row group (same-group pairs always count as NEAR)
    int wrap_first;         // tile_boxes_kernel: frame the wrapped coordinates (raw input spanning 1.4 L or more, ljmd_set_state)
    double L, invL, rc2_skin;   // rc^2 * (1 + 1e-10): skip only when provably outside
    double rsplit2;         // r_split^2
    double rvfar2;          // mixed precision: box distance^2 beyond which a far pass is VERY FAR (u^3 = r^-6 < 2^-26: the u^6
                            // terms lie below the fp32 resolution of the u^3 terms; pair_n3_f32<., VFAR>), or +inf: never
    int pertile_images;     // tile_class: row tiles may take their own periodic image on a single general axis (LJMD_N3_PERTILE)
    int both_ties;          // tile_class: the tie d = NG / 2 is visited from both sides (N3Args::both_ties)
};

// ---- reproducible mode (LJMD_PRECISION_FP64_REPRODUCIBLE): exact fixed-point sums ----
// Every per-pair term t (fx, fy, fz, u^6, u^3) and every v^2 enters as the integer Q(t) = RNE(t 2^64); |t| < 2^40 (else
// the step fails with LJMD_ERR_RANGE), so |Q(t)| < 2^104.  A particle's sum of at most n - 1 < 2^23 terms fits a signed
// 128-bit integer; totals over particles and ranks are 192-bit.  Integer sums do not depend on their order: results
// are a function of the particle set alone.
constexpr int kExactWords = 16;             // int64 words per exact step record (LJMD_EXACT_PARTIAL_WORDS)
constexpr int kFixedQuantities = 5;         // per-particle sums of the pair kernel: ax, ay, az, u^6, u^3
constexpr int kFixedMaxN = 1 << 23;         // largest n of the mode: (n - 1) 2^104 < 2^127
constexpr double kFixedBound = 0x1p40;      // terms must satisfy |t| < kFixedBound
// flags word of an exact record
constexpr int64_t kFlagRange = 1;           // a term was not finite or |t| >= kFixedBound
constexpr int64_t kFlagNoEnergy = 2;        // forces-only evaluation: S12, S6 not summed
constexpr int64_t kFlagNoKinetic = 4;       // no second half-kick: Kx, Ky, Kz not summed

struct FixedArgs {
    const double *pos;      // exchange buffer [G][3][P]
    const uint64_t *mask;   // [TB][W] tile-pair mask (tile_mask_kernel), unused with walk_all
    __int128 *fslab;        // [nslab][kFixedQuantities][P] per-row sums of Q(term) of one column slice
    unsigned *fflag;        // [nslab][TB] 1 = a term of this (slice, row tile) was out of range
    int walk_all;           // 1: every column tile (positions / rc outside the fast path's preconditions)
    int S, P, G, rank, TB, T, W;
    int chunk;              // column tiles per grid.y slice
    int energy;             // 0: forces-only instantiation (u^6, u^3 not summed)
    double L, invL, rc2;
};

struct FixedTailArgs {
    const __int128 *fslab;
    const unsigned *fflag;
    int nslab, P, TB;
    double *a, *v;          // [3][P] of the owned rows
    double dt_half;
    int64_t *blk;           // [P / kBlock][kExactWords] per-block record partials
};

struct FixedFoldArgs {
    const int64_t *blk;
    int n_blk;
    int64_t *rec;           // ring_pos != NULL: ring [ring_cap][kExactWords], record at *ring_pos; else ONE record
    unsigned *ring_pos;
    unsigned ring_cap;
};

// signed 192-bit integers as three little-endian 64-bit limbs (two's complement)
__host__ __device__ inline void add192(uint64_t (&a)[3], const uint64_t (&b)[3])
{
    const uint64_t s0 = a[0] + b[0];
    const uint64_t c0 = s0 < a[0];
    const uint64_t s1 = a[1] + b[1];
    uint64_t c1 = s1 < a[1];
    const uint64_t s1c = s1 + c0;
    c1 += s1c < s1;
    a[2] = a[2] + b[2] + c1;
    a[1] = s1c;
    a[0] = s0;
}

__host__ __device__ inline void from128(uint64_t (&a)[3], __int128 x)
{
    a[0] = (uint64_t)x;
    a[1] = (uint64_t)(x >> 64);
    a[2] = x < 0 ? ~0ull : 0ull;
}

// RNE(x) * 2^-64 for a signed 192-bit x: ONE correctly rounded conversion (the scaling by 2^-64 is exact)
__host__ __device__ inline double fixed_to_double(const uint64_t (&x)[3])
{
    uint64_t m[3] = {x[0], x[1], x[2]};
    const bool neg = (int64_t)m[2] < 0;
    if (neg) {                                      // magnitude: ~m + 1
        m[0] = ~m[0]; m[1] = ~m[1]; m[2] = ~m[2];
        const uint64_t one[3] = {1, 0, 0};
        add192(m, one);
    }
    const int top = m[2] ? 2 : m[1] ? 1 : m[0] ? 0 : -1;
    if (top < 0) return 0.0;
    const int msb = 64 * top + 63 - __builtin_clzll(m[top]);
    auto bits64 = [&](int s) -> uint64_t {         // bits [s, s + 64) of m, s >= 0
        const int w = s >> 6, o = s & 63;
        const uint64_t lo = w < 3 ? m[w] >> o : 0ull;
        const uint64_t hi = (o && w + 1 < 3) ? m[w + 1] << (64 - o) : 0ull;
        return lo | hi;
    };
    double r;
    if (msb <= 52) {
        r = (double)m[0];                           // exact
        r = ldexp(r, -64);
    } else {
        const int sh = msb - 52;                    // bits below the 53-bit significand
        uint64_t mant = bits64(sh) & ((1ull << 53) - 1ull);
        const bool round_bit = (bits64(sh - 1) & 1ull) != 0;
        bool sticky = false;                        // any of the bits [0, sh - 1)
        for (int w = 0; w < 3; ++w) {
            const int b0 = 64 * w, k = sh - 1 - b0;   // bits of word w below sh - 1
            if (k <= 0) break;
            sticky = sticky || (k >= 64 ? m[w] != 0 : (m[w] & ((1ull << k) - 1ull)) != 0);
        }
        if (round_bit && (sticky || (mant & 1ull))) ++mant;   // 2^53 at most: still exact
        r = ldexp((double)mant, sh - 64);
    }
    return neg ? -r : r;
}

struct RdfArgs {
    const double *x, *y, *z;       // [n] one snapshot, wrapped coordinates
    unsigned long long *hist;      // [nbins] ordered-pair counts (added to)
    int n, nbins, chunk;           // chunk = j per grid.y slice
    double L, rmax, dr;
    double invL, inv_dr;           // 1 / L, 1 / dr: fast paths of the two divisions (exact path kept for near-ties)
};

struct TimeOriginArgs {
    const double *x, *y, *z;       // [n_snap][n] unwrapped positions (MSD) or velocities (VACF)
    double *term;                  // [n_origins][max_lag + 1] particle mean per (origin, lag); entries beyond an origin's reach untouched
    int n_snap, n, max_lag, origin_stride;
};

hipError_t launch_pair_rows_generic(const PairArgs &a, dim3 grid, hipStream_t s);
hipError_t launch_pair_tiles(const PairArgs &a, dim3 grid, hipStream_t s);
hipError_t launch_pair_n3(const N3Args &a, dim3 grid, int wg_waves, hipStream_t s);   // dispatches on a.RT, wg_waves
hipError_t launch_pair_n3_f32(const N3Args &a, dim3 grid, hipStream_t s);
hipError_t launch_drift_kick(const IntegrateArgs &a, int phase /* 0 all, 1 positions, 2 velocities */, hipStream_t s);
hipError_t launch_reduce_forces(const ReduceArgs &a, bool all_blocks, hipStream_t s);
hipError_t launch_reduce_forces_split(const ReduceArgs &a, int phase /* 1 or 2 */, hipStream_t s);
hipError_t launch_kick(const IntegrateArgs &a, bool kick, hipStream_t s);
// kick + finalize in one launch: the last block to finish folds the partials (needs a.ticket, f.n_wg <= kDirectFoldMax)
hipError_t launch_kick_finalize(const IntegrateArgs &a, const FinalizeArgs &f, bool kick, hipStream_t s);
hipError_t launch_kinetic_fused(const IntegrateArgs &a, hipStream_t s);
// out[i] = blocks[0][i] + blocks[1][i] + ... + blocks[G-1][i], i < len (left to right: the order is part of the result)
hipError_t launch_sum_blocks(const double *blocks, double *out, int G, int len, hipStream_t s);
hipError_t launch_finalize(const FinalizeArgs &a, double *fold_scratch /* [2 * kFoldBlocks] or NULL */, hipStream_t s);
// small single-rank systems: slab reduction + kick + step record (+ the next step's K1 when drift) in one launch, one
// block per tile; kick without drift = the last step of a batch, neither = a plain force evaluation
hipError_t launch_tile_tail(const ReduceArgs &ra, const IntegrateArgs &a, const FinalizeArgs &f, const FinalizeArgs &prev, bool kick,
                            bool drift, hipStream_t s);
// reproducible mode: pair kernel, then reduction + conversion + x24 (+ kick) with per-block exact partials, then the fold
// of those into one exact record (ring slot or single record); ke_only: the per-block Kx, Ky, Kz of the resident velocities
hipError_t launch_pair_fixed(const FixedArgs &a, dim3 grid, hipStream_t s);
hipError_t launch_fixed_tail(const FixedTailArgs &a, bool kick, bool energy, bool ke_only, hipStream_t s);
hipError_t launch_fixed_fold(const FixedFoldArgs &a, hipStream_t s);
hipError_t launch_rdf_histogram(const RdfArgs &a, dim3 grid, hipStream_t s);
hipError_t launch_time_origin(const TimeOriginArgs &a, bool vacf, int n_origins, hipStream_t s);
hipError_t launch_tile_boxes(const GeometryArgs &a, hipStream_t s);
hipError_t launch_tile_mask(const GeometryArgs &a, hipStream_t s);
hipError_t launch_tile_class(const GeometryArgs &a, double invL, double rc2, int S, int NGo, unsigned *desc,
                             unsigned *desc_far, float *desc2 /* cluster passes, or NULL: none */, hipStream_t s);

// ljmd_sort.hip
size_t kd_temp_bytes(int count);
hipError_t launch_iota(int *idx, int P, hipStream_t s);
hipError_t kd_level(void *temp, size_t temp_bytes, const double *coord_axis, double L, unsigned long long *keys,
                    unsigned long long *keys_out, int *idx, int *idx_out, int S, int nseg, const int *seg_offsets,
                    hipStream_t s);
// ownership migration of a multi-GPU run (ljmd_sort.hip; ljmd_migrate.cpp: migrate_pack / migrate_deal)
constexpr int kMigrateRows = 10;            // doubles per slot in the migration buffer: ru, v, a (3 each) + the particle id
hipError_t launch_iota_blocked(int *idx, int n, int S, int P, hipStream_t s);
hipError_t launch_iota_offset(int *idx, int count, int P, int offset, hipStream_t s);
hipError_t kd_level_blocked(void *temp, size_t temp_bytes, const double *pos, int axis, int P, double L,
                            unsigned long long *keys, unsigned long long *keys_out, int *idx, int *idx_out, int n, int nseg,
                            const int *seg_offsets, hipStream_t s);
hipError_t launch_migrate_pack(const double *ru, const double *v, const double *a, const int *perm, const int *gid0,
                               double *block, int S, int P, hipStream_t s);
hipError_t launch_migrate_select(const double *pos_all, const double *mig_all, const int *mine, double *new_pos, double *ru,
                                 double *v, double *a, int *gid0, int S, int P, hipStream_t s);
// (the launches that finish a re-sort, launch_kd_finish and launch_gather_state: ljmd_sort.h)

// ---- device arithmetic shared by the kernel files ----
// The device functions whose exact sequence of roundings is part of the documented results, ONE copy each for
// ljmd_kernels.hip and the batch kernels (ljmd_batch*.hip): a batch replica equals a single engine bit for bit because
// both compile this text.  It lives in this file, not in a header of its own, because this is one of the two files whose
// hash decides whether a committed profile still describes the kernels (bench.py, tools/pmc_*.py).
// Everything here is built with -ffp-contract=off: FMAs only where the source says fma().

// wave / block reductions with a FIXED combination order: every floating-point sum of the kernels is bitwise
// reproducible run to run.  The only atomics are integer ones that cannot change a result: the blocks-done ticket of
// kick_finalize_kernel and the integer histograms of the g(r) kernels.
__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;  // valid in lane 0
}

// Fixed-order sum of NVAL values per thread over the first W waves of the workgroup, wave w of value k parked at
// lds[k * stride + w].  Every thread of the workgroup calls it (it holds a barrier); waves from W on contribute
// nothing (the batch kernels: W = the replica's own waves).  The result is valid in thread 0.
template <int NVAL>
__device__ __forceinline__ void block_sum(double (&v)[NVAL], double *lds /* [NVAL * stride] */,
                                          int stride = kWavesPerBlock, int W = kWavesPerBlock)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < NVAL; ++k) {
        const double s = wave_sum(v[k]);
        if (lane == 0) lds[k * stride + wave] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < NVAL; ++k) {
            double s = lds[k * stride];
            for (int w = 1; w < W; ++w) s += lds[k * stride + w];
            v[k] = s;
        }
    }
}

// FAST path building blocks.  Preconditions (checked on the host):
//   (a) every coordinate the kernel reads lies within a span < 2.4 L (true after any wrap; the framed copy of the Newton-3
//       kernels, up to L / 2 beyond either end of what it frames, has it for a raw span < 1.4 L and is taken from the
//       wrapped coordinates otherwise: GeometryArgs::wrap_first), so |d/L| < 2.5,
//       n = rndne(d/L) has |n| <= 2 and L*n is exact: fma(-L, n, d) == d - L*n rounded once,
//       i.e. the same value the reference computes;
//   (b) rc <= (1 - 1e-9) L/2: rndne and dnint differ only on exact ties of d/L, where
//       |d_mic| ~ L/2 > rc, so the pair fails r^2 < rc^2 either way.
// Differences from the reference per pair, all <= ~1 ulp of the term: r^2 and the force
// use fma contraction, 1/r^2 is v_rcp_f64 + one Halley step instead of the IEEE divide.
__device__ __forceinline__ double mic_fast(double d, double L, double invL)
{
    return fma(-L, __builtin_rint(d * invL), d);
}

__device__ __forceinline__ double rcp_newton(double x)
{
    // v_rcp_f64 delivers ~24-26 good bits; ONE cubically convergent (Halley) step takes the relative
    // error e to e^3 (< 2^-70): y = y0 (1 + e + e^2), e = 1 - x y0.  3 fma instead of the 4 of two
    // Newton steps; result within 1 ulp of the IEEE quotient (tests/test_gpu_parity.py).
    const double y0 = __builtin_amdgcn_rcp(x);
    const double e = fma(-x, y0, 1.0);
    const double t = fma(e, e, e);
    return fma(y0, t, y0);
}

// ENERGY = false leaves out the two energy sums (forces-only steps of the batch kernel; the forces are the same bits)
template <bool EXCLUDE_SELF, bool ENERGY = true>
__device__ __forceinline__ void pair_fast(double xi, double yi, double zi,
                                          double xj, double yj, double zj,
                                          double L, double invL, double rc2, bool is_self,
                                          double &ax, double &ay, double &az,
                                          double &s12, double &s6)
{
    const double dx = mic_fast(xi - xj, L, invL);
    const double dy = mic_fast(yi - yj, L, invL);
    const double dz = mic_fast(zi - zj, L, invL);
    const double r2 = fma(dz, dz, fma(dy, dy, dx * dx));
    bool in = r2 < rc2;                                  // strict <; NaN (padding, an unused own slot) never passes
    if constexpr (EXCLUDE_SELF) in = in && !is_self;
    if (in) {
        const double u = rcp_newton(r2);
        const double u3 = u * u * u;
        const double u6 = u3 * u3;
        if constexpr (ENERGY) {
            s12 += u6;
            s6 += u3;
        }
        const double g = fma(2.0, u6, -u3) * u;          // = -dU_r * inv_r2
        ax = fma(g, dx, ax);
        ay = fma(g, dy, ay);
        az = fma(g, dz, az);
    }
}

// First half of a velocity-Verlet step for one coordinate of one particle (drift_kick_kernel, tile_tail_kernel, the
// batch kernels), every operation rounded on its own, left to right:
//   r1 = (r0 + v0*dt) + acc*dt_square_half    verlet.f90:58-60
//   r1 = r1 - L*floor(r1*invL)                geometry_pbc.f90:54-56
//   d  = mic(r1 - r0)                         md_simulation_program.f90:341-351 (dnint): what the unwrapped position gains
//   v1 = v0 + acc*dt_half                     verlet.f90:72-74
// In two parts: the callers store r1 and ru + d before they work out v1 (their instruction schedules depend on it), and
// the multi-rank engine runs the two in separate launches (drift_kick_kernel: PHASE).
struct Drift {
    double r1, d;
};
__device__ __forceinline__ Drift drift_wrap(double r0, double v0, double acc, double dt, double dt_sq_half, double L,
                                            double invL)
{
    double r1 = (r0 + v0 * dt) + acc * dt_sq_half;
    r1 = r1 - L * __builtin_floor(r1 * invL);
    double d = r1 - r0;
    d = d - L * __builtin_round(d * invL);
    return {r1, d};
}

__device__ __forceinline__ double half_kick(double v0, double acc, double dt_half) { return v0 + acc * dt_half; }

// g(r) pair pass (rdf_histogram_kernel, batch_rdf_kernel).
// rint(d / L) without the division: d * (1/L) is within 2 ulp of the true quotient, so its nearest integer is the
// reference's unless the product sits within 1e-9 of a half-integer -- then (practically never) the true
// division decides.  Same integer, hence the same bits downstream.
__device__ __forceinline__ double rdf_image(double d, double L, double invL)
{
    const double q = d * invL;
    double n = __builtin_rint(q);
    if (fabs(q - n) > 0.5 - 1e-9) n = __builtin_rint(d / L);
    return n;
}

// int(r / dr): the product with 1/dr decides unless it lands within 1e-9 of an integer
__device__ __forceinline__ int rdf_bin(double r, double dr, double inv_dr)
{
    const double q = r * inv_dr;
    int bin = (int)q;
    if (q - (double)bin < 1e-9 || (double)(bin + 1) - q < 1e-9) bin = (int)(r / dr);
    return bin;
}

// Reproducible mode (above: "exact fixed-point sums").
// acc += Q(t), |t| < 2^40.  v = RNE(t 2^64) is an integer-valued double, |v| < 2^104; split exactly at 2^62:
// hi = trunc(v 2^-62), lo = v - hi 2^62 (|lo| < 2^62, a multiple of ulp(v): representable), both convert exactly.
__device__ __forceinline__ void fixed_add(__int128 &acc, double t)
{
    const double v = __builtin_rint(t * 0x1p64);
    const double hi = __builtin_trunc(v * 0x1p-62);
    const double lo = v - hi * 0x1p62;
    acc += ((__int128)(int64_t)hi << 62) + (__int128)(int64_t)lo;
}

__device__ __forceinline__ bool fixed_out_of_range(double t) { return !(__builtin_fabs(t) < kFixedBound); }

// Per ordered pair the generic kernel's arithmetic -- the reference's own terms -- every term entering its integer sum
template <bool ENERGY>
__device__ __forceinline__ void pair_fixed(double xi, double yi, double zi, double xj, double yj, double zj, double L,
                                           double invL, double rc2, bool is_self, __int128 &ax, __int128 &ay,
                                           __int128 &az, __int128 &s12, __int128 &s6, bool &bad)
{
    const double dx0 = xi - xj, dy0 = yi - yj, dz0 = zi - zj;
    const double dx = dx0 - L * __builtin_round(dx0 * invL);          // geometry_pbc.f90:86
    const double dy = dy0 - L * __builtin_round(dy0 * invL);
    const double dz = dz0 - L * __builtin_round(dz0 * invL);
    const double r2 = dx * dx + dy * dy + dz * dz;                    // lj_potential_energy.f90:129
    if (r2 < rc2 && !is_self) {                                       // :132; NaN (padding, an unused own slot) never passes
        const double u = 1.0 / r2;                                    // :135
        const double u3 = u * u * u;                                  // :136
        const double u6 = u3 * u3;                                    // :137
        const double mdu = 2.0 * u6 - u3;                             // :143
        const double fx = mdu * dx * u, fy = mdu * dy * u, fz = mdu * dz * u;   // :148-155
        // u^3 <= max(1, u^6): the u^6 test covers it, and both instantiations test the same terms
        const bool oob = fixed_out_of_range(fx) || fixed_out_of_range(fy) || fixed_out_of_range(fz) ||
                         fixed_out_of_range(u6);
        bad = bad || oob;
        fixed_add(ax, oob ? 0.0 : fx);
        fixed_add(ay, oob ? 0.0 : fy);
        fixed_add(az, oob ? 0.0 : fz);
        if constexpr (ENERGY) {
            fixed_add(s12, oob ? 0.0 : u6);
            fixed_add(s6, oob ? 0.0 : u3);
        }
    }
}

// Sum of five signed 192-bit values per thread over the first W waves of the workgroup: integer shuffles inside a
// wave, then the waves through LDS.  Every thread of the workgroup calls it (it holds a barrier), waves from W on must
// hold zeros; the result is valid in thread 0.  ROLLED keeps the shuffle tree a loop (the batch kernel, whose pair loop
// leaves no registers to spare); the sum is the same integer either way.
template <bool ROLLED = false>
__device__ __forceinline__ void block_sum192(uint64_t (&q)[5][3], uint64_t (*lds)[5][3] /* [>= W] */,
                                             int W = kWavesPerBlock)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll ROLLED ? 1 : 6
    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            uint64_t o[3];
#pragma unroll
            for (int w = 0; w < 3; ++w) o[w] = __shfl_down(q[k][w], off, 64);
            add192(q[k], o);
        }
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < 5; ++k)
#pragma unroll
            for (int w = 0; w < 3; ++w) lds[wave][k][w] = q[k][w];
    __syncthreads();
    if (threadIdx.x == 0)
        for (int v = 1; v < W; ++v)
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                const uint64_t o[3] = {lds[v][k][0], lds[v][k][1], lds[v][k][2]};
                add192(q[k], o);
            }
}

}  // namespace ljmdk
#endif
