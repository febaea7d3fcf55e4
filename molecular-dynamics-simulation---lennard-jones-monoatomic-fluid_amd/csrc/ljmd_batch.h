// ljmd_batch.h -- argument block of the batch kernel (ljmd_batch.hip), shared with its host side ljmd_batch.cpp.
//
// Device layout of a batch of B replicas, replica b holding n_b particles: twelve planes of offsets[B] = sum n_b
// doubles, the replicas concatenated in replica order inside a plane (element (b, i) at offsets[b] + i; for B replicas
// of one n, offsets[b] = b*n), in the order rx ry rz | ux uy uz | vx vy vz | ax ay az.  Step records: per sample and
// replica kBatchRecWords doubles {0.5 sum u^6, 0.5 sum u^3 over the replica's ordered pairs, sum vx^2, sum vy^2,
// sum vz^2}, sample-major: record (s, b) at (s*B + b) * kBatchRecWords.
#ifndef LJMD_BATCH_KERNEL_H
#define LJMD_BATCH_KERNEL_H

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <type_traits>

namespace ljmdb {

constexpr int kBatchRecWords = 5;
constexpr int kBatchMaxThreads = 1024;                 // 16 waves: one workgroup per replica
constexpr int kBatchMaxWaves = kBatchMaxThreads / 64;

enum BatchMode : int {
    kModeForces = 0,    // t = 0 evaluation: a = 24 f, energy sums into record 0 (no drift, no kick)
    kModeSteps = 1,     // nsteps x { drift + wrap + half-kick + unwrapped update ; pair forces ; half-kick }
    kModeKinetic = 2,   // record 0 word 2 = sum (vx*vx + vy*vy + vz*vz), the fused form of ljmd_kinetic_energy
};

// one replica of a launch: its own n and constants.  The host keeps these entries grouped by kernel class
// (batch_class); a launch covers a contiguous range of them, blockIdx.x + BatchArgs::g0.
struct BatchReplica {
    size_t off;             // offsets[b]: the replica's first element in every plane
    int b;                  // replica index: its record slot
    int n;
    int threads;            // batch_threads(n): the replica's own thread count, <= blockDim.x
    int pad_;
    double L, invL, rc2, dt, dt_half, dt_sq_half;
};

struct BatchArgs {
    double *state;          // [12][plane]
    double *rec;            // [n_samples][B][kBatchRecWords]
    const BatchReplica *rep;  // the handle's replica table (device), launch order
    size_t B;               // replicas of the handle (record stride)
    size_t plane;           // elements of one plane = offsets[B]
    int g0;                 // first table entry of this launch (blockIdx.x + g0)
    int mode;
    int nsteps;             // steps of this launch (kModeSteps)
    int step0;              // steps of the same ljmd_batch_steps call before this launch
    int sample_every;       // step s (1-based within the call) is sampled when s % sample_every == 0; 0 = none
};

// own particles per thread: 1 up to n = 1024, then 2, then 4 (<= 1024 threads per workgroup)
inline int batch_k(int n) { return n <= 1024 ? 1 : n <= 2048 ? 2 : 4; }
inline int batch_threads(int n)
{
    const int k = batch_k(n);
    return 64 * ((n + 64 * k - 1) / (64 * k));
}

// kernel class (NMAX, K) of a replica of n particles: 0 <= 128 < 1 <= 512 < 2 <= 1024 < 3 <= 2048 < 4 <= 4096
constexpr int kBatchClasses = 5;
inline int batch_class(int n) { return n <= 128 ? 0 : n <= 512 ? 1 : n <= 1024 ? 2 : n <= 2048 ? 3 : 4; }

// The classes in one place, for the kernel files: f(NMAX, K) -- both as std::integral_constant -- launches the caller's
// kernel of the class of n_max.
template <typename F>
hipError_t dispatch_class(int n_max, int n_blocks, F &&f)
{
    if (n_max <= 0 || n_max > 4096 || n_blocks <= 0) return hipErrorInvalidValue;
    auto launch = [&](auto nmax, auto k) {
        static_assert(64 * ((nmax() + 64 * k() - 1) / (64 * k())) <= kBatchMaxThreads, "too many threads for the class");
        f(nmax, k);
        return hipGetLastError();
    };
    using std::integral_constant;
    switch (batch_class(n_max)) {
    case 0: return launch(integral_constant<int, 128>{}, integral_constant<int, 1>{});
    case 1: return launch(integral_constant<int, 512>{}, integral_constant<int, 1>{});
    case 2: return launch(integral_constant<int, 1024>{}, integral_constant<int, 1>{});
    case 3: return launch(integral_constant<int, 2048>{}, integral_constant<int, 2>{});
    default: return launch(integral_constant<int, 4096>{}, integral_constant<int, 4>{});
    }
}

// one launch of n_blocks table entries, all of batch_class(n_max), each at most n_max particles; the workgroup has
// batch_threads(n_max) threads, of which an entry of fewer particles uses its own batch_threads(n)
hipError_t launch_batch(const BatchArgs &a, int n_max, int n_blocks, hipStream_t s);

// The same launch in the reproducible mode (ljmd_batch_fixed.hip).  b.rec is not used: the step records are exact,
// LJMD_EXACT_PARTIAL_WORDS int64 words per (sample, replica) in the layout of ljmd_read_partials_exact -- S12 and S6
// over the replica's ORDERED pairs, to be halved as integers -- record (s, b) at (s*B + b) * LJMD_EXACT_PARTIAL_WORDS.
struct BatchFixedArgs {
    BatchArgs b;
    int64_t *rec;           // [n_samples][B][LJMD_EXACT_PARTIAL_WORDS]
    int32_t *range;         // [B] sticky: set to 1 when a term of replica b was out of range, never cleared by a kernel
};
hipError_t launch_batch_fixed(const BatchFixedArgs &a, int n_max, int n_blocks, hipStream_t s);

// g(r) accumulation (ljmd_batch_rdf.hip): the pair-distance histogram of every replica's resident positions, added to
// the replica's row of hist.  Same launch geometry as launch_batch; the kernel class sets only the LDS of the positions.
constexpr int kBatchRdfMaxBins = 8192;                 // 32 KiB of 32-bit LDS bins beside <= 96 KiB of positions
struct BatchRdfReplica {    // entry b of the handle's second table, replica order
    double rmax, dr, inv_dr;  // dr = rmax / nbins, inv_dr = 1 / dr
};
struct BatchRdfArgs {
    const double *r;        // [3][plane]: the wrapped positions (planes rx ry rz of the state)
    const BatchReplica *rep;
    const BatchRdfReplica *rdf;   // [B]
    unsigned long long *hist;     // [B][nbins], row b written by replica b's workgroup alone
    size_t plane;
    int g0;
    int nbins;
};
hipError_t launch_batch_rdf(const BatchRdfArgs &a, int n_max, int n_blocks, hipStream_t s);

// The time-origin observables, MSD / VACF (ljmd_batch_tcf.hip) and van Hove (ljmd_batch_vanhove.h): one snapshot -- every
// replica's resident state -- against the live origins of the ring, the exact integer sums of Q(term) added to the
// replica's rows of sums; the snapshot is then stored as an origin when its number is a multiple of the origin stride.
// Same launch geometry as launch_batch.  The host derives the live origins from the snapshot number s: origin e = 0 ..
// n_live - 1 is the snapshot t0 = t0_first + e * stride, at lag s - t0 = lag_first - e * stride (1 <= lag <= max_lag), in
// ring slot (slot_first + e) % slots; with the newest origin at lag 1 its lag-0 terms are added too.
struct BatchOriginArgs {
    const double *state;    // [12][plane]: ru = planes 3..5, v = planes 6..8
    double *ring;           // [slots][C][plane]: the C components of the stored origins -- 6: ru and v, 3: ru alone
    uint64_t *sums;         // [B][2][max_lag + 1][3] signed 192-bit, two kinds; replica b's rows are written by its
                            // workgroup alone
    int32_t *range;         // [B] sticky: set to 1 when a term of replica b was out of range
    const BatchReplica *rep;
    size_t plane;
    int g0;
    int max_lag, stride, slots;
    int n_live, lag_first, slot_first;
    int store_slot;         // ring slot that takes this snapshot, or -1: not an origin
};

// the checks a launch makes of its window, against the observable's limits
inline bool batch_origin_window_ok(const BatchOriginArgs &a, int max_lag, int max_origins)
{
    if (a.max_lag < 1 || a.max_lag > max_lag || a.stride < 1 || a.slots < 1 || a.slots > max_origins || a.n_live < 0 ||
        a.n_live > a.slots || a.slot_first < 0 || a.slot_first >= a.slots || a.store_slot >= a.slots)
        return false;
    return a.n_live == 0 || (a.lag_first <= a.max_lag && a.lag_first - (a.n_live - 1) * a.stride >= 1);
}

// MSD / VACF: the ring holds ru and v, kind 0 = MSD, 1 = VACF
constexpr int kBatchTcfMaxLag = 4096;                  // LJMD_BATCH_TCF_MAX_LAG
constexpr int kBatchTcfMaxOrigins = 512;               // LJMD_BATCH_TCF_MAX_ORIGINS: ring slots = max_lag / stride + 1
using BatchTcfArgs = BatchOriginArgs;
hipError_t launch_batch_tcf(const BatchTcfArgs &a, int n_max, int n_blocks, hipStream_t s);

// A series of snapshots of exact integer sums -- the pressure tensor (ljmd_batch_stress.h) and the heat flux
// (ljmd_batch_heatflux.h): one snapshot of every replica of a launch, the replica's resident wrapped r and v -> its sums
// in row (row, b) of the series, the workgroup being that row's only writer.  Same launch geometry as launch_batch.
struct BatchSeriesArgs {
    const double *state;    // [12][plane]: r = planes 0..2, v = planes 6..8
    uint64_t *words;        // [rows][B][words of the observable] signed 192-bit, sample-major
    int32_t *range;         // [B] sticky: set to 1 when a pair or a particle of replica b was out of range
    const BatchReplica *rep;
    size_t plane;
    size_t B;               // replicas of the handle (row stride)
    int64_t row;            // snapshot this launch writes, 0 <= row < rows
    int64_t rows;           // snapshots the series holds
    int g0;
};
using BatchSeriesLauncher = hipError_t (*)(const BatchSeriesArgs &a, int n_max, int n_blocks, hipStream_t s);

}  // namespace ljmdb

#endif  // LJMD_BATCH_KERNEL_H
