// ljmd_batch_host.h -- what the host files of the batch engine share (ljmd_batch.cpp: lifecycle, planning, step loop;
// ljmd_batch_rdf.cpp: g(r); ljmd_batch_origins.cpp: the one core of the time-origin observables, driven by the
// descriptors of ljmd_batch_tcf.cpp: MSD / VACF, and ljmd_vanhove_batch.cpp: van Hove; ljmd_batch_series.cpp: the one
// core of the series observables, driven by the descriptors of ljmd_stress_batch.cpp: pressure tensor, and
// ljmd_heatflux_batch.cpp: heat flux; ljmd_rhok_batch.cpp: the density modes, a core of its own): the handle, the entry
// guard, the poison and allocation helpers, and the form in which the step loop sees an accumulator.  Host code only; the
// kernels' side is ljmd_batch.h.
#ifndef LJMD_BATCH_HOST_H
#define LJMD_BATCH_HOST_H

#include "ljmd_batch.h"
#include "ljmd_common.h"
#include "ljmd_internal.h"

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

struct ljmd_batch;

namespace ljmdb __attribute__((visibility("hidden"))) {   // host-only: no symbol of libljmd.so

// one replica's parameters and derived constants (host side)
struct BatchRep : ljmdh::SimParams {
    int n = 0;
};

// the replicas of one kernel class: entries [first, first + count) of the replica table, launched chunk replicas and
// steps_per_launch steps at a time (launch_shape of n_max, the group's largest n)
struct BatchGroup {
    size_t first = 0, count = 0;
    int n_max = 0;
    size_t chunk = 0;
    int steps_per_launch = 0;
    size_t rdf_chunk = 0;             // replicas per g(r) launch: launch_shape's pair bound of the fp64 mode, one step
    hipStream_t stream = nullptr;     // own stream when the handle runs its groups concurrently, else the handle's
    hipEvent_t done = nullptr;
};

// g(r) accumulation (ljmd_batch_rdf.cpp): off while nbins == 0, and every is 0 then
struct BatchRdf {
    int32_t nbins = 0, every = 0;
    int64_t snapshots = 0;
    unsigned long long *d_hist = nullptr;   // [B][nbins]
    BatchRdfReplica *d_table = nullptr;     // [B], replica order
};

// An accumulator as the step loop sees it (run_groups, ljmd_batch_steps): a launch ends at the steps every, 2 every, ...
// of the call, the group's enqueue follows it on the same stream, and ran() does the host's share after the whole call.
struct BatchAccumulator {
    int every = 0;                    // steps between two snapshots of ljmd_batch_steps; 0: off, or not taken by it
    const char *name = nullptr;       // "g(r)": "... is not a multiple of the g(r) interval"
    const char *tag = nullptr;        // "rdf": ljmd_batch_rdf_configure
    // the launches of group g on stream s for snapshot k (0-based) of this call; counts them; a failure poisons
    int (*enqueue)(ljmd_batch *h, const BatchGroup &g, hipStream_t s, int k, int32_t *count, const char *who) = nullptr;
    void (*ran)(ljmd_batch *h, int snapshots) = nullptr;
    // NULL, or whether the `snapshots` of a call fit: LJMD_OK, or LJMD_ERR_STATE before anything is launched
    int (*room)(ljmd_batch *h, int snapshots, const char *who) = nullptr;
};

// a series of snapshots of exact integer sums -- the pressure tensor's (ljmd_stress_batch.cpp) and the heat flux's
// (ljmd_heatflux_batch.cpp), both through ljmd_batch_series.cpp: off while max_snapshots == 0, and every is 0 then.
// Those two files are not linked into every program that links ljmd_batch.cpp (tests/batch_trace), so the handle carries
// their entry into the step loop and their release: ljmd_batch_stress_configure / ljmd_batch_heatflux_configure fill
// both, and default-constructed means nothing is called
struct BatchSeries {
    int32_t max_snapshots = 0, every = 0;
    int64_t count = 0;                // snapshots in the series
    uint64_t *d_words = nullptr;      // [max_snapshots][B][sums][3] signed 192-bit: 12 sums (stress), 9 (heat flux)
    int32_t *d_range = nullptr;       // [B] sticky until ljmd_batch_stress_reset / ljmd_batch_heatflux_reset
    BatchAccumulator acc;
    void (*release)(ljmd_batch *h) = nullptr;
};
using BatchStress = BatchSeries;
using BatchHeatflux = BatchSeries;

// A time-origin observable -- MSD / VACF (ljmd_batch_tcf.cpp) and van Hove (ljmd_vanhove_batch.cpp), both through
// ljmd_batch_origins.cpp: off while max_lag == 0, and every is 0 then.  Without a histogram (MSD / VACF) nbins stays 0 and
// d_hist and d_dr NULL.  acc and release (default-constructed: nothing is called) are how the step loop and
// ljmd_batch_destroy reach van Hove, whose file is not linked everywhere; MSD / VACF: tcf_accumulator, tcf_release.
struct BatchOrigins {
    int32_t max_lag = 0, stride = 1, every = 0, slots = 0, nbins = 0;
    int64_t s = 0;                    // number of the next snapshot of this trajectory (0 after ljmd_batch_set_state)
    int64_t snapshots = 0;            // snapshots since configure / reset, over all trajectories
    std::vector<int64_t> counts;      // [max_lag + 1] origins that contributed to each lag: the same for all replicas
    unsigned long long *d_hist = nullptr;   // [B][max_lag + 1][nbins + 1]
    uint64_t *d_sums = nullptr;       // [B][2][max_lag + 1][3] signed 192-bit: MSD then VACF, or S2 then S4
    int32_t *d_range = nullptr;       // [B] sticky until ljmd_batch_tcf_reset / ljmd_batch_vanhove_reset
    double *d_dr = nullptr;           // [2][B]: dr_b = rmax[b] / nbins, then 1 / dr_b
    double *d_ring = nullptr;         // [slots][6 or 3][offsets[B]]: the stored origins
    BatchAccumulator acc;
    void (*release)(ljmd_batch *h) = nullptr;
};
using BatchTcf = BatchOrigins;
using BatchVanhove = BatchOrigins;

// the density modes rho_k (ljmd_rhok_batch.cpp, a core of its own: the snapshot's width 6 n_modes is set at run time):
// off while max_snapshots == 0, and every is 0 then.  acc and release (default-constructed: nothing is called) are how
// the step loop and ljmd_batch_destroy reach the file, which is not linked everywhere
struct BatchRhok {
    int32_t max_snapshots = 0, every = 0, n_modes = 0;
    int waves = 0;                    // waves of a workgroup of the kernel (LJMD_BATCH_RHOK_WAVES; else kBatchRhokWaves)
    int64_t count = 0;                // snapshots in the series
    uint64_t *d_words = nullptr;      // [max_snapshots][B][n_modes][6] signed 192-bit: Re then Im
    int32_t *d_modes = nullptr;       // [n_modes][3]
    int32_t *d_range = nullptr;       // [B] sticky until ljmd_batch_rhok_reset
    hipEvent_t ev[2] = {nullptr, nullptr};   // around the launches of the last ljmd_batch_rhok_accumulate
    bool timed = false;
    BatchAccumulator acc;
    void (*release)(ljmd_batch *h) = nullptr;
};

}  // namespace ljmdb

struct ljmd_batch {
    size_t B = 0;
    size_t total = 0;                 // offsets[B]: elements of one plane
    int device = 0;
    std::vector<ljmdb::BatchRep> rep; // [B], replica order
    std::vector<int64_t> offsets;     // [B + 1]
    std::vector<ljmdb::BatchGroup> groups;   // by kernel class, ascending
    bool concurrent = false;          // groups on streams of their own, joined before the records are fetched
    int mode = LJMD_PRECISION_FP64;   // or LJMD_PRECISION_FP64_REPRODUCIBLE (ljmd_batch_set_precision)
    bool tail_on = true;
    bool have_state = false, have_accel = false;
    bool poisoned = false;            // a launch failed half-way: LJMD_ERR_STATE until ljmd_batch_set_state
    hipStream_t stream = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    hipEvent_t fork = nullptr;
    ljmdb::BatchReplica *d_table = nullptr;  // [B], the groups' entries one after another
    double *d_state = nullptr;        // [12][offsets[B]]
    double *d_rec = nullptr;          // [samples][B][rec_words]: doubles, or int64 words in the reproducible mode
    size_t rec_cap = 0;               // 8-byte words the record buffer holds (>= B * kExactWords)
    std::vector<double> h_rec;
    int32_t *d_range = nullptr;       // [B] reproducible mode: sticky range flags, cleared by ljmd_batch_set_state
    std::vector<int32_t> h_range;
    double last_ms = 0.0;             // kernel time of the last ljmd_batch_steps call
    int32_t last_launches = 0;
    ljmdb::BatchRdf rdf;
    ljmdb::BatchTcf tcf;
    ljmdb::BatchStress stress;
    ljmdb::BatchHeatflux heatflux;
    ljmdb::BatchVanhove vanhove;
    ljmdb::BatchRhok rhok;
    std::string err;
};

namespace ljmdb __attribute__((visibility("hidden"))) {

using ljmdh::fail;

inline bool reproducible(const ljmd_batch *h) { return h->mode == LJMD_PRECISION_FP64_REPRODUCIBLE; }
inline double *plane(ljmd_batch *h, int which, int axis) { return h->d_state + ((size_t)which * 3 + axis) * h->total; }

// What an entry point requires before it starts, checked in this order after the NULL handle: configured g(r),
// configured MSD / VACF, configured pressure tensor, configured heat flux, configured van Hove, configured density
// modes, a state, valid accelerations, no poison (LJMD_ERR_STATE each); kNeedDevice: the handle's device is then made
// current (ljmd_batch.cpp)
enum BatchNeed : unsigned { kNeedRdf = 1, kNeedTcf = 2, kNeedState = 4, kNeedAccel = 8, kNeedSound = 16, kNeedDevice = 32,
                         kNeedStress = 64, kNeedHeatflux = 128, kNeedVanhove = 256, kNeedRhok = 512 };
int enter(ljmd_batch *h, const char *who, unsigned need);

// fails the call as fail() does and poisons the handle: LJMD_ERR_STATE from the guarded calls until ljmd_batch_set_state
inline int poison(ljmd_batch *h, int code, const char *fmt, ...)
{
    h->poisoned = true;
    va_list ap;
    va_start(ap, fmt);
    ljmdh::failv(&h->err, code, fmt, ap);
    va_end(ap);
    return code;
}

// `bytes` of device memory in *p, or *p = NULL and "<who>: cannot allocate <bytes> bytes of <what>"
template <class T>
int device_alloc(ljmd_batch *h, T **p, size_t bytes, const char *who, const char *what)
{
    if (hipMalloc(p, bytes) == hipSuccess) return LJMD_OK;
    *p = nullptr;
    return fail(h, LJMD_ERR_ALLOC, "%s: cannot allocate %zu bytes of %s", who, bytes, what);
}

// grow() sizes host containers; std::bad_alloc becomes "<who>: out of host memory" (h may be NULL)
template <class F>
int host_alloc(const ljmd_batch *h, const char *who, F &&grow)
{
    try {
        grow();
    } catch (const std::bad_alloc &) {
        return fail(h, LJMD_ERR_ALLOC, "%s: out of host memory", who);
    }
    return LJMD_OK;
}

BatchAccumulator rdf_accumulator(const ljmd_batch *h);    // ljmd_batch_rdf.cpp
BatchAccumulator tcf_accumulator(const ljmd_batch *h);    // ljmd_batch_tcf.cpp
using BatchAccumulators = std::array<BatchAccumulator, 6>;
inline BatchAccumulators accumulators(const ljmd_batch *h)     // the newest last: the earlier launch sequences are unchanged
{
    BatchAccumulator stress = h->stress.acc, heatflux = h->heatflux.acc, vanhove = h->vanhove.acc, rhok = h->rhok.acc;
    stress.every = h->stress.every;
    heatflux.every = h->heatflux.every;
    vanhove.every = h->vanhove.every;
    rhok.every = h->rhok.every;
    return {rdf_accumulator(h), tcf_accumulator(h), stress, heatflux, vanhove, rhok};
}

// one snapshot of the resident state outside ljmd_batch_steps, on the handle's stream (ljmd_batch_*_accumulate)
int accumulate_now(ljmd_batch *h, const BatchAccumulator &a, const char *who);

// frees what ljmd_batch_*_configure allocated and switches the accumulator off (ljmd_batch_destroy)
void rdf_release(ljmd_batch *h);
void tcf_release(ljmd_batch *h);

// What ljmd_batch_series.cpp is driven by: one constant per series observable (ljmd_stress_batch.cpp,
// ljmd_heatflux_batch.cpp).  The core references no launcher itself, so it links into every program that links
// ljmd_batch*.cpp.  acc and release are what configure leaves in the handle's BatchSeries: the observable's entries into
// the step loop, which pass this descriptor and its own series on to series_enqueue / series_room / series_release.
struct BatchSeriesDesc {
    BatchSeries ljmd_batch::*series;  // &ljmd_batch::stress: the observable's series of a handle
    BatchAccumulator acc;             // name "pressure tensor", tag "stress", enqueue, ran, room; every = 0
    void (*release)(ljmd_batch *h);
    int words;                        // int64 words of one (snapshot, replica)
    int max_snapshots;                // LJMD_BATCH_*_MAX_SNAPSHOTS
    unsigned need;                    // kNeedStress
    BatchSeriesLauncher launch;
};
int series_enqueue(ljmd_batch *h, const BatchSeriesDesc &d, const BatchGroup &g, hipStream_t s, int k, int32_t *count,
                   const char *who);
int series_room(ljmd_batch *h, const BatchSeriesDesc &d, int snapshots, const char *who);
void series_release(ljmd_batch *h, const BatchSeriesDesc &d);
// the bodies of ljmd_batch_<tag>_configure / _accumulate / _read_exact / _reset; `who` = the public name, h may be NULL
int series_configure(ljmd_batch *h, const BatchSeriesDesc &d, int32_t max_snapshots, int32_t every, const char *who);
int series_accumulate(ljmd_batch *h, const BatchSeriesDesc &d, const char *who);
// the guards (a poisoned handle may still be read), the series so far in words -- waits for the device; a set range word
// fails the call and names the lowest such replica
int series_fetch(ljmd_batch *h, const BatchSeriesDesc &d, int64_t *words, int64_t *n_snapshots, const char *who);
// the start of a read in doubles: the guard, then series_fetch into *w, sized here, when `want`
int series_read_words(ljmd_batch *h, const BatchSeriesDesc &d, bool want, std::vector<int64_t> *w, int64_t *n_snapshots,
                      const char *who);
int series_reset(ljmd_batch *h, const BatchSeriesDesc &d, const char *who);


// What ljmd_batch_origins.cpp is driven by: one constant per time-origin observable.  The core references no launcher
// itself, so it links into every program that links ljmd_batch*.cpp.  acc and release pass this descriptor on to
// origins_enqueue / origins_ran / origins_release; configure leaves them in the handle's BatchOrigins.
struct BatchOriginDesc {
    BatchOrigins ljmd_batch::*state;  // &ljmd_batch::tcf: the observable's state of a handle
    unsigned need;                    // kNeedTcf
    int components;                   // of a ring slot: 6 (ru and v) or 3 (ru alone)
    int max_lag, max_origins, max_bins;   // LJMD_BATCH_*_MAX_LAG, _MAX_ORIGINS, _MAX_BINS; max_bins == 0: no histogram
    const char *phrase;               // "MSD / VACF": "(0 switches MSD / VACF off)"
    const char *limits;               // "TCF": "exceeds LJMD_BATCH_TCF_MAX_ORIGINS"
    const char *range;                // what a set range word means: "replica 1: <range>; the flag stays until ..."
    bool range_first;                 // a set range word fails a read before anything is written, not after everything is
    BatchAccumulator acc;             // name "MSD / VACF", tag "tcf", enqueue, ran; every = 0
    void (*release)(ljmd_batch *h);
    // the observable's own launcher on the common block `a` of the state `q`
    hipError_t (*launch)(const ljmd_batch *h, const BatchOrigins &q, const BatchOriginArgs &a, int n_max, int n_blocks,
                         hipStream_t s);
};
int origins_enqueue(ljmd_batch *h, const BatchOriginDesc &d, const BatchGroup &g, hipStream_t s, int k, int32_t *count,
                    const char *who);
void origins_ran(ljmd_batch *h, const BatchOriginDesc &d, int snapshots);
void origins_release(ljmd_batch *h, const BatchOriginDesc &d);
// ljmd_batch_<tag>_configure in two parts (`who` = the public name, h may be NULL): the entry and the shared guards; then,
// behind the observable's own guards, the device, the release and the buffers.  dr: the [2][B] bin widths with a histogram
int origins_configure_guards(ljmd_batch *h, const BatchOriginDesc &d, int32_t max_lag, int32_t origin_stride, int32_t every,
                             const char *who);
int origins_configure(ljmd_batch *h, const BatchOriginDesc &d, int32_t max_lag, int32_t origin_stride, int32_t every,
                      int32_t nbins, const double *dr, const char *who);
// the bodies of ljmd_batch_<tag>_accumulate / _read / _read_exact / _reset; hist is NULL without a histogram
int origins_accumulate(ljmd_batch *h, const BatchOriginDesc &d, const char *who);
int origins_read(ljmd_batch *h, const BatchOriginDesc &d, uint64_t *hist, double *kind0, double *kind1, int64_t *counts,
                 int64_t *n_snapshots, const char *who);
int origins_read_exact(ljmd_batch *h, const BatchOriginDesc &d, uint64_t *hist, int64_t *words, int64_t *counts,
                       int64_t *n_snapshots, const char *who);
int origins_reset(ljmd_batch *h, const BatchOriginDesc &d, const char *who);

}  // namespace ljmdb
#endif
