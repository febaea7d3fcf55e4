// ljmd_batch_origins.cpp -- the one host core of the batch engine's time-origin observables, MSD / VACF
// (ljmd_batch_tcf.cpp) and the van Hove self-correlation (ljmd_vanhove_batch.cpp): the numbering of the snapshots and the
// ring of origins, configure / accumulate / read / reset of a BatchOrigins of the handle and its launches from the step
// loop, driven by the observable's BatchOriginDesc (ljmd_batch_host.h).  The window, the counts and the quotient are
// those of ljmd_tcf_host.h.  No launcher is referenced here -- the descriptor carries it -- so this file links into every
// program that links ljmd_batch*.cpp with launchers of its own (tests/batch_trace, tests/prepare_host).
#include "ljmd_batch_host.h"
#include "ljmd_tcf_host.h"

namespace ljmdb {

using ljmdh::tcf_count;
using ljmdh::tcf_quotient;
using ljmdh::tcf_window;
using ljmdh::TcfWindow;

namespace {

// Snapshot s: its live origins are the multiples t0 of the stride with 1 <= s - t0 <= max_lag (BatchOriginArgs);
// n_live == 0 and store_slot < 0: nothing to launch
TcfWindow window(const BatchOrigins &q, int64_t s) { return tcf_window(s, q.max_lag, q.stride, q.slots); }

size_t rows(const BatchOrigins &q) { return (size_t)q.max_lag + 1; }
size_t hist_words(const ljmd_batch *h, const BatchOrigins &q) { return h->B * rows(q) * ((size_t)q.nbins + 1); }
size_t sum_words(const ljmd_batch *h, const BatchOrigins &q) { return h->B * 2 * rows(q) * 3; }

// a set range word fails a read and names the lowest such replica.  No poison, unlike the range flag of the reproducible
// mode (fetch_records): the trajectory itself is sound
int range_set(ljmd_batch *h, const BatchOriginDesc &d, int64_t flagged, const char *who)
{
    if (flagged < 0) return LJMD_OK;
    return fail(h, LJMD_ERR_RANGE, "%s: replica %lld: %s; the flag stays until ljmd_batch_%s_reset", who, (long long)flagged,
                d.range, d.acc.tag);
}

// What origins_read and origins_read_exact share: the guards (a poisoned handle may still be read), the device's
// histogram in hist and sums in h_words -- waits for the device -- and the host's counts.  *flagged: the lowest replica
// whose range word is set, or -1; the caller fills its arrays and then fails the call (range_set) -- unless the observable
// fails it here, before anything is written to the caller's arrays (BatchOriginDesc::range_first)
int fetch(ljmd_batch *h, const BatchOriginDesc &d, uint64_t *hist, std::vector<uint64_t> *h_words, int64_t *counts,
          int64_t *n_snapshots, int64_t *flagged, const char *who)
{
    LJMD_TRY(enter(h, who, d.need | kNeedDevice));
    const BatchOrigins &q = h->*d.state;
    std::vector<int32_t> range;
    LJMD_TRY(host_alloc(h, who, [&] {
        range.resize(h->B);
        if (h_words) h_words->resize(sum_words(h, q));
    }));
    static_assert(sizeof(uint64_t) == sizeof(unsigned long long), "histogram word");
    hipError_t e = hipMemcpyAsync(range.data(), q.d_range, h->B * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess && hist && q.d_hist)
        e = hipMemcpyAsync(hist, q.d_hist, hist_words(h, q) * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess && h_words)
        e = hipMemcpyAsync(h_words->data(), q.d_sums, h_words->size() * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream);
    const hipError_t s = hipStreamSynchronize(h->stream);
    if (e != hipSuccess || s != hipSuccess)
        return poison(h, LJMD_ERR_HIP, "%s: kernel or copy failed: %s; the handle is poisoned until ljmd_batch_set_state",
                      who, hipGetErrorString(e != hipSuccess ? e : s));
    *flagged = -1;
    for (size_t b = 0; b < h->B && *flagged < 0; ++b)
        if (range[b] != 0) *flagged = (int64_t)b;
    if (d.range_first) LJMD_TRY(range_set(h, d, *flagged, who));
    if (counts) std::copy(q.counts.begin(), q.counts.end(), counts);
    if (n_snapshots) *n_snapshots = q.snapshots;
    return LJMD_OK;
}

}  // namespace

// the launch of group g on stream s_: the resident state as snapshot number s + k -- one launch per group (the caller
// advances the numbering once every group is enqueued: origins_ran)
int origins_enqueue(ljmd_batch *h, const BatchOriginDesc &d, const BatchGroup &g, hipStream_t s_, int k, int32_t *count,
                    const char *who)
{
    const BatchOrigins &q = h->*d.state;
    const TcfWindow w = window(q, q.s + k);
    if (w.n_live == 0 && w.store_slot < 0) return LJMD_OK;
    BatchOriginArgs a{};
    a.state = h->d_state;
    a.ring = q.d_ring;
    a.sums = q.d_sums;
    a.range = q.d_range;
    a.rep = h->d_table;
    a.plane = h->total;
    a.g0 = (int)g.first;
    a.max_lag = q.max_lag;
    a.stride = q.stride;
    a.slots = q.slots;
    a.n_live = w.n_live;
    a.lag_first = w.lag_first;
    a.slot_first = w.slot_first;
    a.store_slot = w.store_slot;
    const hipError_t e = d.launch(h, q, a, g.n_max, (int)g.count, s_);
    ++*count;
    if (e != hipSuccess)
        return poison(h, LJMD_ERR_HIP, "%s: %s launch failed: %s; the handle is poisoned until ljmd_batch_set_state", who,
                      d.acc.name, hipGetErrorString(e));
    return LJMD_OK;
}

// the host's share of `snapshots` snapshots, once every group's launches are enqueued: the counts and the numbering
void origins_ran(ljmd_batch *h, const BatchOriginDesc &d, int snapshots)
{
    BatchOrigins &q = h->*d.state;
    for (int k = 0; k < snapshots; ++k) {
        tcf_count(window(q, q.s), q.stride, q.counts.data());
        ++q.s;
        ++q.snapshots;
    }
}

// releases the buffers after what may still use them, and switches the feature off
void origins_release(ljmd_batch *h, const BatchOriginDesc &d)
{
    BatchOrigins &q = h->*d.state;
    if (h->stream && (q.d_hist || q.d_sums || q.d_range || q.d_dr || q.d_ring)) (void)hipStreamSynchronize(h->stream);
    if (q.d_hist) (void)hipFree(q.d_hist);
    if (q.d_sums) (void)hipFree(q.d_sums);
    if (q.d_range) (void)hipFree(q.d_range);
    if (q.d_dr) (void)hipFree(q.d_dr);
    if (q.d_ring) (void)hipFree(q.d_ring);
    q = {};
}

int origins_configure_guards(ljmd_batch *h, const BatchOriginDesc &d, int32_t max_lag, int32_t origin_stride, int32_t every,
                             const char *who)
{
    LJMD_TRY(enter(h, who, 0));
    if (max_lag < 0 || max_lag > d.max_lag)
        return fail(h, LJMD_ERR_INVALID_ARG, "%s: max_lag = %d outside 1..%d (0 switches %s off)", who, max_lag, d.max_lag,
                    d.phrase);
    if (every < 0) return fail(h, LJMD_ERR_INVALID_ARG, "%s: every must be >= 0", who);
    if (max_lag > 0 && origin_stride < 1) return fail(h, LJMD_ERR_INVALID_ARG, "%s: origin_stride must be >= 1", who);
    if (max_lag > 0 && max_lag / origin_stride + 1 > d.max_origins)
        return fail(h, LJMD_ERR_INVALID_ARG, "%s: max_lag / origin_stride + 1 = %d exceeds LJMD_BATCH_%s_MAX_ORIGINS (%d)", who,
                    max_lag / origin_stride + 1, d.limits, d.max_origins);
    return LJMD_OK;
}

int origins_configure(ljmd_batch *h, const BatchOriginDesc &d, int32_t max_lag, int32_t origin_stride, int32_t every,
                      int32_t nbins, const double *dr, const char *who)
{
    LJMD_HIP(h, hipSetDevice(h->device));
    origins_release(h, d);
    if (max_lag == 0) return LJMD_OK;
    BatchOrigins &q = h->*d.state;
    const int32_t slots = max_lag / origin_stride + 1;
    const size_t nrows = (size_t)max_lag + 1;
    const size_t hbytes = h->B * nrows * ((size_t)nbins + 1) * sizeof(uint64_t), sbytes = h->B * 2 * nrows * 3 * sizeof(uint64_t);
    const size_t fbytes = h->B * sizeof(int32_t), dbytes = 2 * h->B * sizeof(double);
    const size_t rbytes = (size_t)slots * d.components * h->total * sizeof(double);
    char ring[48];
    std::snprintf(ring, sizeof ring, "the origin ring (%d slots)", slots);
    auto body = [&]() -> int {
        LJMD_TRY(host_alloc(h, who, [&] { q.counts.assign(nrows, 0); }));
        if (d.max_bins) LJMD_TRY(device_alloc(h, &q.d_hist, hbytes, who, "the histogram"));
        LJMD_TRY(device_alloc(h, &q.d_sums, sbytes, who, "sums"));
        LJMD_TRY(device_alloc(h, &q.d_range, fbytes, who, "range words"));
        if (d.max_bins) LJMD_TRY(device_alloc(h, &q.d_dr, dbytes, who, "bin widths"));
        LJMD_TRY(device_alloc(h, &q.d_ring, rbytes, who, ring));
        if (d.max_bins) LJMD_HIP(h, hipMemsetAsync(q.d_hist, 0, hbytes, h->stream));
        LJMD_HIP(h, hipMemsetAsync(q.d_sums, 0, sbytes, h->stream));
        LJMD_HIP(h, hipMemsetAsync(q.d_range, 0, fbytes, h->stream));
        LJMD_HIP(h, hipMemsetAsync(q.d_ring, 0, rbytes, h->stream));
        if (!d.max_bins) return LJMD_OK;   // no wait, unlike ljmd_batch_rdf_configure: nothing here is read from host memory
        LJMD_HIP(h, hipMemcpyAsync(q.d_dr, dr, dbytes, hipMemcpyHostToDevice, h->stream));
        LJMD_HIP(h, hipStreamSynchronize(h->stream));      // dr is read from host memory that ends with this call
        return LJMD_OK;
    };
    const int rc_ = body();
    if (rc_ != LJMD_OK) {
        (void)hipGetLastError();       // a failed hipMalloc is otherwise what the next launch returns (dispatch_class);
        origins_release(h, d);         // ljmd_batch_rdf_configure does not clear it -- kept as it is
        return rc_;
    }
    q.max_lag = max_lag;
    q.stride = origin_stride;
    q.every = every;
    q.slots = slots;
    q.nbins = d.max_bins ? nbins : 0;
    q.acc = d.acc;
    q.release = d.release;
    return LJMD_OK;
}

int origins_accumulate(ljmd_batch *h, const BatchOriginDesc &d, const char *who)
{
    LJMD_TRY(enter(h, who, d.need | kNeedState | kNeedSound | kNeedDevice));
    return accumulate_now(h, d.acc, who);
}

int origins_read(ljmd_batch *h, const BatchOriginDesc &d, uint64_t *hist, double *kind0, double *kind1, int64_t *counts,
                 int64_t *n_snapshots, const char *who)
{
    std::vector<uint64_t> w;
    int64_t flagged = -1;
    LJMD_TRY(fetch(h, d, hist, kind0 || kind1 ? &w : nullptr, counts, n_snapshots, &flagged, who));
    const BatchOrigins &q = h->*d.state;
    const size_t nrows = rows(q);
    double *const dst[2] = {kind0, kind1};
    for (size_t b = 0; b < h->B; ++b)
        for (int kind = 0; kind < 2; ++kind)
            for (size_t l = 0; dst[kind] && l < nrows; ++l) {
                uint64_t x[3];
                std::memcpy(x, w.data() + ((b * 2 + kind) * nrows + l) * 3, sizeof x);
                dst[kind][b * nrows + l] = tcf_quotient(x, h->rep[b].n, q.counts[l]);    // what ljmd_tcf_from_exact computes
            }
    return range_set(h, d, flagged, who);
}

int origins_read_exact(ljmd_batch *h, const BatchOriginDesc &d, uint64_t *hist, int64_t *words, int64_t *counts,
                       int64_t *n_snapshots, const char *who)
{
    std::vector<uint64_t> w;
    int64_t flagged = -1;
    LJMD_TRY(fetch(h, d, hist, words ? &w : nullptr, counts, n_snapshots, &flagged, who));
    if (words) std::memcpy(words, w.data(), w.size() * sizeof(uint64_t));
    return range_set(h, d, flagged, who);
}

int origins_reset(ljmd_batch *h, const BatchOriginDesc &d, const char *who)
{
    LJMD_TRY(enter(h, who, d.need | kNeedDevice));
    BatchOrigins &q = h->*d.state;
    if (q.d_hist) LJMD_HIP(h, hipMemsetAsync(q.d_hist, 0, hist_words(h, q) * sizeof(uint64_t), h->stream));
    LJMD_HIP(h, hipMemsetAsync(q.d_sums, 0, sum_words(h, q) * sizeof(uint64_t), h->stream));
    LJMD_HIP(h, hipMemsetAsync(q.d_range, 0, h->B * sizeof(int32_t), h->stream));
    std::fill(q.counts.begin(), q.counts.end(), 0);
    q.s = 0;
    q.snapshots = 0;
    return LJMD_OK;
}

}  // namespace ljmdb
