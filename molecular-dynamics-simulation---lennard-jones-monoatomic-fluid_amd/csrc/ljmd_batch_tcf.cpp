// ljmd_batch_tcf.cpp -- host side of the batch engine's MSD / VACF accumulation (include/ljmd.h: ljmd_batch_tcf_*,
// ljmd_tcf_from_exact; kernel: ljmd_batch_tcf.hip): configure / accumulate / read / reset, the numbering of the
// snapshots and the ring of origins, and the entry through which the step loop of ljmd_batch.cpp takes its snapshots.
#include "ljmd_batch_host.h"
#include "ljmd_tcf_host.h"

using namespace ljmdb;
using ljmdh::tcf_count;
using ljmdh::tcf_quotient;
using ljmdh::tcf_window;
using ljmdh::TcfWindow;

static_assert(kBatchTcfMaxLag == LJMD_BATCH_TCF_MAX_LAG && kBatchTcfMaxOrigins == LJMD_BATCH_TCF_MAX_ORIGINS,
              "MSD / VACF limits out of sync with include/ljmd.h");

namespace {

// The launch arguments of snapshot s, but for the group.  Its live origins are the multiples t0 of the stride with
// 1 <= s - t0 <= max_lag (BatchTcfArgs); n_live == 0 and store_slot < 0: nothing to launch
BatchTcfArgs tcf_snapshot(const ljmd_batch *h, int64_t s)
{
    const TcfWindow w = tcf_window(s, h->tcf.max_lag, h->tcf.stride, h->tcf.slots);
    BatchTcfArgs ta{};
    ta.state = h->d_state;
    ta.ring = h->tcf.d_ring;
    ta.sums = h->tcf.d_sums;
    ta.range = h->tcf.d_range;
    ta.rep = h->d_table;
    ta.plane = h->total;
    ta.max_lag = h->tcf.max_lag;
    ta.stride = h->tcf.stride;
    ta.slots = h->tcf.slots;
    ta.n_live = w.n_live;
    ta.lag_first = w.lag_first;
    ta.slot_first = w.slot_first;
    ta.store_slot = w.store_slot;
    return ta;
}

// the MSD / VACF launch of group g on stream s_: the resident ru and v as snapshot number tcf.s + k -- one launch per
// group (the caller advances the numbering once every group is enqueued: tcf_ran)
int enqueue_tcf(ljmd_batch *h, const BatchGroup &g, hipStream_t s_, int k, int32_t *count, const char *who)
{
    BatchTcfArgs ta = tcf_snapshot(h, h->tcf.s + k);
    if (ta.n_live == 0 && ta.store_slot < 0) return LJMD_OK;
    ta.g0 = (int)g.first;
    const hipError_t e = launch_batch_tcf(ta, g.n_max, (int)g.count, s_);
    ++*count;
    if (e != hipSuccess)
        return poison(h, LJMD_ERR_HIP, "%s: MSD / VACF launch failed: %s; the handle is poisoned until ljmd_batch_set_state",
                      who, hipGetErrorString(e));
    return LJMD_OK;
}

// the host's share of `snapshots` snapshots, once every group's launches are enqueued: the counts and the numbering
void tcf_ran(ljmd_batch *h, int snapshots)
{
    for (int k = 0; k < snapshots; ++k) {
        tcf_count(tcf_window(h->tcf.s, h->tcf.max_lag, h->tcf.stride, h->tcf.slots), h->tcf.stride, h->tcf.counts.data());
        ++h->tcf.s;
        ++h->tcf.snapshots;
    }
}

size_t tcf_sum_words(const ljmd_batch *h) { return h->B * 2 * ((size_t)h->tcf.max_lag + 1) * 3; }

// what ljmd_batch_tcf_read and ljmd_batch_tcf_read_exact share: the guards (a poisoned handle may still be read), the
// device's sums in h_words -- waits for the device; a set range word fails the call and names the lowest such replica --
// and the host's counts
int tcf_fetch(ljmd_batch *h, std::vector<uint64_t> *h_words, int64_t *counts, int64_t *n_snapshots, const char *who)
{
    LJMD_TRY(enter(h, who, kNeedTcf | kNeedDevice));
    std::vector<int32_t> range;
    LJMD_TRY(host_alloc(h, who, [&] {
        range.resize(h->B);
        if (h_words) h_words->resize(tcf_sum_words(h));
    }));
    hipError_t e = hipMemcpyAsync(range.data(), h->tcf.d_range, h->B * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess && h_words)
        e = hipMemcpyAsync(h_words->data(), h->tcf.d_sums, h_words->size() * sizeof(uint64_t), hipMemcpyDeviceToHost,
                           h->stream);
    const hipError_t s = hipStreamSynchronize(h->stream);
    if (e != hipSuccess || s != hipSuccess)
        return poison(h, LJMD_ERR_HIP, "%s: kernel or copy failed: %s; the handle is poisoned until ljmd_batch_set_state",
                      who, hipGetErrorString(e != hipSuccess ? e : s));
    // no poison, unlike the range flag of the reproducible mode (fetch_records): the trajectory itself is sound
    for (size_t b = 0; b < h->B; ++b)
        if (range[b] != 0)
            return fail(h, LJMD_ERR_RANGE, "%s: replica %zu: an MSD or VACF term was not finite or |term| >= 2^40 and "
                                           "entered as 0; the flag stays until ljmd_batch_tcf_reset", who, b);
    if (counts) std::copy(h->tcf.counts.begin(), h->tcf.counts.end(), counts);
    if (n_snapshots) *n_snapshots = h->tcf.snapshots;
    return LJMD_OK;
}

}  // namespace

BatchAccumulator ljmdb::tcf_accumulator(const ljmd_batch *h)
{
    return {h->tcf.every, "MSD / VACF", "tcf", enqueue_tcf, tcf_ran};
}

// releases the MSD / VACF buffers after what may still use them
void ljmdb::tcf_release(ljmd_batch *h)
{
    if (h->stream && (h->tcf.d_sums || h->tcf.d_range || h->tcf.d_ring)) (void)hipStreamSynchronize(h->stream);
    if (h->tcf.d_sums) (void)hipFree(h->tcf.d_sums);
    if (h->tcf.d_range) (void)hipFree(h->tcf.d_range);
    if (h->tcf.d_ring) (void)hipFree(h->tcf.d_ring);
    h->tcf = {};
}

extern "C" {

int ljmd_batch_tcf_configure(ljmd_batch_t *h, int32_t max_lag, int32_t origin_stride, int32_t every)
{
    static const char *who = "ljmd_batch_tcf_configure";
    LJMD_TRY(enter(h, who, 0));
    if (max_lag < 0 || max_lag > kBatchTcfMaxLag)
        return fail(h, LJMD_ERR_INVALID_ARG, "%s: max_lag = %d outside 1..%d (0 switches MSD / VACF off)", who, max_lag,
                     kBatchTcfMaxLag);
    if (every < 0) return fail(h, LJMD_ERR_INVALID_ARG, "%s: every must be >= 0", who);
    if (max_lag > 0 && origin_stride < 1) return fail(h, LJMD_ERR_INVALID_ARG, "%s: origin_stride must be >= 1", who);
    if (max_lag > 0 && max_lag / origin_stride + 1 > kBatchTcfMaxOrigins)
        return fail(h, LJMD_ERR_INVALID_ARG, "%s: max_lag / origin_stride + 1 = %d exceeds LJMD_BATCH_TCF_MAX_ORIGINS "
                                              "(%d)", who, max_lag / origin_stride + 1, kBatchTcfMaxOrigins);
    LJMD_HIP(h, hipSetDevice(h->device));
    tcf_release(h);
    if (max_lag == 0) return LJMD_OK;
    const int32_t slots = max_lag / origin_stride + 1;
    const size_t sbytes = h->B * 2 * ((size_t)max_lag + 1) * 3 * sizeof(uint64_t), fbytes = h->B * sizeof(int32_t);
    const size_t rbytes = (size_t)slots * 6 * h->total * sizeof(double);
    char ring[48];
    std::snprintf(ring, sizeof ring, "the origin ring (%d slots)", slots);
    auto body = [&]() -> int {
        LJMD_TRY(host_alloc(h, who, [&] { h->tcf.counts.assign((size_t)max_lag + 1, 0); }));
        LJMD_TRY(device_alloc(h, &h->tcf.d_sums, sbytes, who, "sums"));
        LJMD_TRY(device_alloc(h, &h->tcf.d_range, fbytes, who, "range words"));
        LJMD_TRY(device_alloc(h, &h->tcf.d_ring, rbytes, who, ring));
        LJMD_HIP(h, hipMemsetAsync(h->tcf.d_sums, 0, sbytes, h->stream));
        LJMD_HIP(h, hipMemsetAsync(h->tcf.d_range, 0, fbytes, h->stream));
        LJMD_HIP(h, hipMemsetAsync(h->tcf.d_ring, 0, rbytes, h->stream));
        return LJMD_OK;                // no wait, unlike ljmd_batch_rdf_configure: nothing here is read from host memory
    };
    const int rc_ = body();
    if (rc_ != LJMD_OK) {
        (void)hipGetLastError();       // a failed hipMalloc is otherwise what the next launch returns (dispatch_class);
        tcf_release(h);                // ljmd_batch_rdf_configure does not clear it -- kept as it is
        return rc_;
    }
    h->tcf.max_lag = max_lag;
    h->tcf.stride = origin_stride;
    h->tcf.every = every;
    h->tcf.slots = slots;
    return LJMD_OK;
}

int ljmd_batch_tcf_accumulate(ljmd_batch_t *h)
{
    static const char *who = "ljmd_batch_tcf_accumulate";
    LJMD_TRY(enter(h, who, kNeedTcf | kNeedState | kNeedSound | kNeedDevice));
    return accumulate_now(h, tcf_accumulator(h), who);
}

int ljmd_tcf_from_exact(const int64_t *words, int32_t n, int64_t count, double *out)
{
    if (!words || !out) return fail(nullptr, LJMD_ERR_INVALID_ARG, "ljmd_tcf_from_exact: NULL argument");
    if (n < 1 || count < 0) return fail(nullptr, LJMD_ERR_INVALID_ARG, "ljmd_tcf_from_exact: n must be >= 1, count >= 0");
    const uint64_t x[3] = {(uint64_t)words[0], (uint64_t)words[1], (uint64_t)words[2]};
    *out = tcf_quotient(x, n, count);
    return LJMD_OK;
}

int ljmd_batch_tcf_read(ljmd_batch_t *h, double *msd, double *vacf, int64_t *counts, int64_t *n_snapshots)
{
    static const char *who = "ljmd_batch_tcf_read";
    std::vector<uint64_t> w;
    LJMD_TRY(tcf_fetch(h, msd || vacf ? &w : nullptr, counts, n_snapshots, who));
    const size_t rows = (size_t)h->tcf.max_lag + 1;
    double *const dst[2] = {msd, vacf};
    for (size_t b = 0; b < h->B; ++b)
        for (int kind = 0; kind < 2; ++kind)
            for (size_t l = 0; dst[kind] && l < rows; ++l) {
                int64_t x[3];
                std::memcpy(x, w.data() + ((b * 2 + kind) * rows + l) * 3, sizeof x);
                (void)ljmd_tcf_from_exact(x, h->rep[b].n, h->tcf.counts[l], dst[kind] + b * rows + l);
            }
    return LJMD_OK;
}

int ljmd_batch_tcf_read_exact(ljmd_batch_t *h, int64_t *words, int64_t *counts, int64_t *n_snapshots)
{
    static const char *who = "ljmd_batch_tcf_read_exact";
    std::vector<uint64_t> w;
    LJMD_TRY(tcf_fetch(h, words ? &w : nullptr, counts, n_snapshots, who));
    if (words) std::memcpy(words, w.data(), w.size() * sizeof(uint64_t));
    return LJMD_OK;
}

int ljmd_batch_tcf_reset(ljmd_batch_t *h)
{
    static const char *who = "ljmd_batch_tcf_reset";
    LJMD_TRY(enter(h, who, kNeedTcf | kNeedDevice));
    LJMD_HIP(h, hipMemsetAsync(h->tcf.d_sums, 0, tcf_sum_words(h) * sizeof(uint64_t), h->stream));
    LJMD_HIP(h, hipMemsetAsync(h->tcf.d_range, 0, h->B * sizeof(int32_t), h->stream));
    std::fill(h->tcf.counts.begin(), h->tcf.counts.end(), 0);
    h->tcf.s = 0;
    h->tcf.snapshots = 0;
    return LJMD_OK;
}

}  // extern "C"
