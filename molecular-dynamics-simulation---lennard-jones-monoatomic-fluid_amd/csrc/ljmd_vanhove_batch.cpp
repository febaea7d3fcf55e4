// ljmd_vanhove_batch.cpp -- host side of the batch engine's van Hove self-correlation (include/ljmd.h:
// ljmd_batch_vanhove_*; kernel: ljmd_batch_vanhove.hip): configure / accumulate / read / reset, the numbering of the
// snapshots and the ring of origins -- the window, the counts and the quotient are those of ljmd_tcf_host.h, called as
// ljmd_batch_tcf.cpp calls them -- and the entry through which the step loop of ljmd_batch.cpp takes its snapshots.
// The file name does not match ljmd_batch*.cpp on purpose, as ljmd_stress_batch.cpp's and ljmd_heatflux_batch.cpp's: the
// host transcripts of the batch engine (tests/batch_trace/Makefile and its like) link every such file with launchers of
// their own and have none for this kernel.  So ljmd_batch.cpp references no symbol of this file:
// ljmd_batch_vanhove_configure leaves the accumulator and the release in the handle (BatchVanhove), which is how the step
// loop and ljmd_batch_destroy reach them.
#include "ljmd_batch_host.h"
#include "ljmd_batch_vanhove.h"
#include "ljmd_tcf_host.h"

using namespace ljmdb;
using ljmdh::tcf_count;
using ljmdh::tcf_quotient;
using ljmdh::tcf_window;
using ljmdh::TcfWindow;

static_assert(kBatchVanhoveMaxLag == LJMD_BATCH_VANHOVE_MAX_LAG && kBatchVanhoveMaxOrigins == LJMD_BATCH_VANHOVE_MAX_ORIGINS &&
                  kBatchVanhoveMaxBins == LJMD_BATCH_VANHOVE_MAX_BINS, "van Hove limits out of sync with include/ljmd.h");

namespace {

size_t vh_rows(const ljmd_batch *h) { return (size_t)h->vanhove.max_lag + 1; }
size_t vh_hist_words(const ljmd_batch *h) { return h->B * vh_rows(h) * ((size_t)h->vanhove.nbins + 1); }
size_t vh_sum_words(const ljmd_batch *h) { return h->B * 2 * vh_rows(h) * 3; }

TcfWindow vh_window(const ljmd_batch *h, int64_t s)
{
    return tcf_window(s, h->vanhove.max_lag, h->vanhove.stride, h->vanhove.slots);
}

// the van Hove launch of group g on stream s_: the resident ru as snapshot number vanhove.s + k -- one launch per group
// (the caller advances the numbering once every group is enqueued: vh_ran)
int vh_enqueue(ljmd_batch *h, const BatchGroup &g, hipStream_t s_, int k, int32_t *count, const char *who)
{
    const BatchVanhove &v = h->vanhove;
    const TcfWindow w = vh_window(h, v.s + k);
    if (w.n_live == 0 && w.store_slot < 0) return LJMD_OK;
    BatchVanhoveArgs a{};
    a.state = h->d_state;
    a.ring = v.d_ring;
    a.hist = v.d_hist;
    a.sums = v.d_sums;
    a.range = v.d_range;
    a.dr = v.d_dr;
    a.inv_dr = v.d_dr + h->B;
    a.rep = h->d_table;
    a.plane = h->total;
    a.g0 = (int)g.first;
    a.nbins = v.nbins;
    a.max_lag = v.max_lag;
    a.stride = v.stride;
    a.slots = v.slots;
    a.n_live = w.n_live;
    a.lag_first = w.lag_first;
    a.slot_first = w.slot_first;
    a.store_slot = w.store_slot;
    const hipError_t e = launch_batch_vanhove(a, g.n_max, (int)g.count, s_);
    ++*count;
    if (e != hipSuccess)
        return poison(h, LJMD_ERR_HIP, "%s: van Hove launch failed: %s; the handle is poisoned until ljmd_batch_set_state",
                      who, hipGetErrorString(e));
    return LJMD_OK;
}

// the host's share of `snapshots` snapshots, once every group's launches are enqueued: the counts and the numbering
void vh_ran(ljmd_batch *h, int snapshots)
{
    for (int k = 0; k < snapshots; ++k) {
        tcf_count(vh_window(h, h->vanhove.s), h->vanhove.stride, h->vanhove.counts.data());
        ++h->vanhove.s;
        ++h->vanhove.snapshots;
    }
}

// releases the van Hove buffers after what may still use them, and switches the feature off
void vh_release(ljmd_batch *h)
{
    BatchVanhove &v = h->vanhove;
    if (h->stream && (v.d_hist || v.d_sums || v.d_range || v.d_dr || v.d_ring)) (void)hipStreamSynchronize(h->stream);
    if (v.d_hist) (void)hipFree(v.d_hist);
    if (v.d_sums) (void)hipFree(v.d_sums);
    if (v.d_range) (void)hipFree(v.d_range);
    if (v.d_dr) (void)hipFree(v.d_dr);
    if (v.d_ring) (void)hipFree(v.d_ring);
    v = {};
}

// what ljmd_batch_vanhove_read and ljmd_batch_vanhove_read_exact share: the guards (a poisoned handle may still be read),
// the device's histogram in hist and sums in h_words -- waits for the device -- and the host's counts.  *flagged: the
// lowest replica whose range word is set, or -1; the caller fills its arrays and then fails the call (vh_range)
int vh_fetch(ljmd_batch *h, uint64_t *hist, std::vector<uint64_t> *h_words, int64_t *counts, int64_t *n_snapshots,
             int64_t *flagged, const char *who)
{
    LJMD_TRY(enter(h, who, kNeedVanhove | kNeedDevice));
    const BatchVanhove &v = h->vanhove;
    std::vector<int32_t> range;
    LJMD_TRY(host_alloc(h, who, [&] {
        range.resize(h->B);
        if (h_words) h_words->resize(vh_sum_words(h));
    }));
    hipError_t e = hipMemcpyAsync(range.data(), v.d_range, h->B * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess && hist)
        e = hipMemcpyAsync(hist, v.d_hist, vh_hist_words(h) * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess && h_words)
        e = hipMemcpyAsync(h_words->data(), v.d_sums, h_words->size() * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream);
    const hipError_t s = hipStreamSynchronize(h->stream);
    if (e != hipSuccess || s != hipSuccess)
        return poison(h, LJMD_ERR_HIP, "%s: kernel or copy failed: %s; the handle is poisoned until ljmd_batch_set_state",
                      who, hipGetErrorString(e != hipSuccess ? e : s));
    if (counts) std::copy(v.counts.begin(), v.counts.end(), counts);
    if (n_snapshots) *n_snapshots = v.snapshots;
    *flagged = -1;
    for (size_t b = 0; b < h->B && *flagged < 0; ++b)
        if (range[b] != 0) *flagged = (int64_t)b;
    return LJMD_OK;
}

// no poison, as the MSD / VACF range word (tcf_fetch): the trajectory itself is sound
int vh_range(ljmd_batch *h, int64_t flagged, const char *who)
{
    if (flagged < 0) return LJMD_OK;
    return fail(h, LJMD_ERR_RANGE, "%s: replica %lld: a van Hove displacement was not finite or r^4 >= 2^40: it was counted "
                                   "in the overflow column and entered the sums as 0; the flag stays until "
                                   "ljmd_batch_vanhove_reset", who, (long long)flagged);
}

}  // namespace

extern "C" {

int ljmd_batch_vanhove_configure(ljmd_batch_t *h, int32_t max_lag, int32_t origin_stride, int32_t nbins, const double *rmax,
                                 int32_t every)
{
    static const char *who = "ljmd_batch_vanhove_configure";
    LJMD_TRY(enter(h, who, 0));
    if (max_lag < 0 || max_lag > kBatchVanhoveMaxLag)
        return fail(h, LJMD_ERR_INVALID_ARG, "%s: max_lag = %d outside 1..%d (0 switches the van Hove function off)", who,
                     max_lag, kBatchVanhoveMaxLag);
    if (every < 0) return fail(h, LJMD_ERR_INVALID_ARG, "%s: every must be >= 0", who);
    if (max_lag > 0 && origin_stride < 1) return fail(h, LJMD_ERR_INVALID_ARG, "%s: origin_stride must be >= 1", who);
    if (max_lag > 0 && max_lag / origin_stride + 1 > kBatchVanhoveMaxOrigins)
        return fail(h, LJMD_ERR_INVALID_ARG, "%s: max_lag / origin_stride + 1 = %d exceeds LJMD_BATCH_VANHOVE_MAX_ORIGINS "
                                              "(%d)", who, max_lag / origin_stride + 1, kBatchVanhoveMaxOrigins);
    std::vector<double> dr;
    if (max_lag > 0) {
        if (nbins < 1 || nbins > kBatchVanhoveMaxBins)
            return fail(h, LJMD_ERR_INVALID_ARG, "%s: nbins = %d outside 1..%d", who, nbins, kBatchVanhoveMaxBins);
        if (!rmax) return fail(h, LJMD_ERR_INVALID_ARG, "%s: rmax is NULL", who);
        LJMD_TRY(host_alloc(h, who, [&] { dr.resize(2 * h->B); }));
        for (size_t b = 0; b < h->B; ++b) {
            if (!std::isfinite(rmax[b]) || !(rmax[b] > 0.0))
                return fail(h, LJMD_ERR_INVALID_ARG, "%s: replica %zu: rmax must be finite and > 0", who, b);
            dr[b] = rmax[b] / (double)nbins;
            if (!std::isnormal(dr[b]))
                return fail(h, LJMD_ERR_INVALID_ARG, "%s: replica %zu: rmax / nbins is not a normal number", who, b);
            dr[h->B + b] = 1.0 / dr[b];
        }
    }
    LJMD_HIP(h, hipSetDevice(h->device));
    vh_release(h);
    if (max_lag == 0) return LJMD_OK;
    BatchVanhove &v = h->vanhove;
    const int32_t slots = max_lag / origin_stride + 1;
    const size_t rows = (size_t)max_lag + 1;
    const size_t hbytes = h->B * rows * ((size_t)nbins + 1) * sizeof(uint64_t), sbytes = h->B * 2 * rows * 3 * sizeof(uint64_t);
    const size_t fbytes = h->B * sizeof(int32_t), dbytes = 2 * h->B * sizeof(double);
    const size_t rbytes = (size_t)slots * 3 * h->total * sizeof(double);
    char ring[48];
    std::snprintf(ring, sizeof ring, "the origin ring (%d slots)", slots);
    auto body = [&]() -> int {
        LJMD_TRY(host_alloc(h, who, [&] { v.counts.assign(rows, 0); }));
        LJMD_TRY(device_alloc(h, &v.d_hist, hbytes, who, "the histogram"));
        LJMD_TRY(device_alloc(h, &v.d_sums, sbytes, who, "sums"));
        LJMD_TRY(device_alloc(h, &v.d_range, fbytes, who, "range words"));
        LJMD_TRY(device_alloc(h, &v.d_dr, dbytes, who, "bin widths"));
        LJMD_TRY(device_alloc(h, &v.d_ring, rbytes, who, ring));
        LJMD_HIP(h, hipMemsetAsync(v.d_hist, 0, hbytes, h->stream));
        LJMD_HIP(h, hipMemsetAsync(v.d_sums, 0, sbytes, h->stream));
        LJMD_HIP(h, hipMemsetAsync(v.d_range, 0, fbytes, h->stream));
        LJMD_HIP(h, hipMemsetAsync(v.d_ring, 0, rbytes, h->stream));
        LJMD_HIP(h, hipMemcpyAsync(v.d_dr, dr.data(), dbytes, hipMemcpyHostToDevice, h->stream));
        LJMD_HIP(h, hipStreamSynchronize(h->stream));      // dr is read from host memory that ends with this call
        return LJMD_OK;
    };
    const int rc_ = body();
    if (rc_ != LJMD_OK) {
        (void)hipGetLastError();       // a failed hipMalloc is otherwise what the next launch returns (dispatch_class)
        vh_release(h);
        return rc_;
    }
    v.max_lag = max_lag;
    v.stride = origin_stride;
    v.every = every;
    v.slots = slots;
    v.nbins = nbins;
    v.acc = {0, "van Hove", "vanhove", vh_enqueue, vh_ran, nullptr};
    v.release = vh_release;
    return LJMD_OK;
}

int ljmd_batch_vanhove_accumulate(ljmd_batch_t *h)
{
    static const char *who = "ljmd_batch_vanhove_accumulate";
    LJMD_TRY(enter(h, who, kNeedVanhove | kNeedState | kNeedSound | kNeedDevice));
    return accumulate_now(h, h->vanhove.acc, who);
}

int ljmd_batch_vanhove_read(ljmd_batch_t *h, uint64_t *hist, double *r2, double *r4, int64_t *counts, int64_t *n_snapshots)
{
    static const char *who = "ljmd_batch_vanhove_read";
    std::vector<uint64_t> w;
    int64_t flagged = -1;
    LJMD_TRY(vh_fetch(h, hist, r2 || r4 ? &w : nullptr, counts, n_snapshots, &flagged, who));
    const size_t rows = vh_rows(h);
    double *const dst[2] = {r2, r4};
    for (size_t b = 0; b < h->B; ++b)
        for (int kind = 0; kind < 2; ++kind)
            for (size_t l = 0; dst[kind] && l < rows; ++l) {
                uint64_t x[3];
                std::memcpy(x, w.data() + ((b * 2 + kind) * rows + l) * 3, sizeof x);
                dst[kind][b * rows + l] = tcf_quotient(x, h->rep[b].n, h->vanhove.counts[l]);
            }
    return vh_range(h, flagged, who);
}

int ljmd_batch_vanhove_read_exact(ljmd_batch_t *h, uint64_t *hist, int64_t *words, int64_t *counts, int64_t *n_snapshots)
{
    static const char *who = "ljmd_batch_vanhove_read_exact";
    std::vector<uint64_t> w;
    int64_t flagged = -1;
    LJMD_TRY(vh_fetch(h, hist, words ? &w : nullptr, counts, n_snapshots, &flagged, who));
    if (words) std::memcpy(words, w.data(), w.size() * sizeof(uint64_t));
    return vh_range(h, flagged, who);
}

int ljmd_batch_vanhove_reset(ljmd_batch_t *h)
{
    static const char *who = "ljmd_batch_vanhove_reset";
    LJMD_TRY(enter(h, who, kNeedVanhove | kNeedDevice));
    BatchVanhove &v = h->vanhove;
    LJMD_HIP(h, hipMemsetAsync(v.d_hist, 0, vh_hist_words(h) * sizeof(uint64_t), h->stream));
    LJMD_HIP(h, hipMemsetAsync(v.d_sums, 0, vh_sum_words(h) * sizeof(uint64_t), h->stream));
    LJMD_HIP(h, hipMemsetAsync(v.d_range, 0, h->B * sizeof(int32_t), h->stream));
    std::fill(v.counts.begin(), v.counts.end(), 0);
    v.s = 0;
    v.snapshots = 0;
    return LJMD_OK;
}

}  // extern "C"
