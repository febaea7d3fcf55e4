// ljmd_batch_series.cpp -- the one host core of the batch engine's series observables, the pressure tensor
// (ljmd_stress_batch.cpp) and the heat flux (ljmd_heatflux_batch.cpp): configure / accumulate / fetch / reset of a
// BatchSeries of the handle and its launches from the step loop, driven by the observable's BatchSeriesDesc
// (ljmd_batch_host.h).  No launcher is referenced here -- the descriptor carries it -- so this file links into every
// program that links ljmd_batch*.cpp with launchers of its own (tests/batch_trace, tests/prepare_host).
#include "ljmd_batch_host.h"

namespace ljmdb {

namespace {

size_t row_words(const ljmd_batch *h, const BatchSeriesDesc &d) { return h->B * (size_t)d.words; }

}  // namespace

// the launches of group g on stream s for snapshot k of a call: row count + k of the series, chunks of at most rdf_chunk
// replicas (launch_shape's pair bound of the fp64 mode, one step)
int series_enqueue(ljmd_batch *h, const BatchSeriesDesc &d, const BatchGroup &g, hipStream_t s, int k, int32_t *count,
                   const char *who)
{
    const BatchSeries &q = h->*d.series;
    BatchSeriesArgs sa{};
    sa.state = h->d_state;
    sa.words = q.d_words;
    sa.range = q.d_range;
    sa.rep = h->d_table;
    sa.plane = h->total;
    sa.B = h->B;
    sa.row = q.count + k;
    sa.rows = q.max_snapshots;
    for (size_t c0 = 0; c0 < g.count; c0 += g.rdf_chunk) {
        sa.g0 = (int)(g.first + c0);
        const hipError_t e = d.launch(sa, g.n_max, (int)std::min(g.rdf_chunk, g.count - c0), s);
        ++*count;
        if (e != hipSuccess)
            return poison(h, LJMD_ERR_HIP, "%s: %s launch failed: %s; the handle is poisoned until ljmd_batch_set_state", who,
                          d.acc.name, hipGetErrorString(e));
    }
    return LJMD_OK;
}

int series_room(ljmd_batch *h, const BatchSeriesDesc &d, int snapshots, const char *who)
{
    const BatchSeries &q = h->*d.series;
    if (q.count + snapshots <= q.max_snapshots) return LJMD_OK;
    return fail(h, LJMD_ERR_STATE, "%s: the %s series is full: %lld of %d snapshots taken, %d more do not fit "
                                   "(read it, then ljmd_batch_%s_reset)", who, d.acc.name, (long long)q.count,
                q.max_snapshots, snapshots, d.acc.tag);
}

// releases the series after what may still use it and switches the feature off
void series_release(ljmd_batch *h, const BatchSeriesDesc &d)
{
    BatchSeries *q = &(h->*d.series);
    if (h->stream && (q->d_words || q->d_range)) (void)hipStreamSynchronize(h->stream);
    if (q->d_words) (void)hipFree(q->d_words);
    if (q->d_range) (void)hipFree(q->d_range);
    *q = {};
}

int series_fetch(ljmd_batch *h, const BatchSeriesDesc &d, int64_t *words, int64_t *n_snapshots, const char *who)
{
    LJMD_TRY(enter(h, who, d.need | kNeedDevice));
    const BatchSeries &q = h->*d.series;
    std::vector<int32_t> range;
    LJMD_TRY(host_alloc(h, who, [&] { range.resize(h->B); }));
    hipError_t e = hipMemcpyAsync(range.data(), q.d_range, h->B * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess && words && q.count > 0)
        e = hipMemcpyAsync(words, q.d_words, (size_t)q.count * row_words(h, d) * sizeof(uint64_t), hipMemcpyDeviceToHost,
                           h->stream);
    const hipError_t s = hipStreamSynchronize(h->stream);
    if (e != hipSuccess || s != hipSuccess)
        return poison(h, LJMD_ERR_HIP, "%s: kernel or copy failed: %s; the handle is poisoned until ljmd_batch_set_state",
                      who, hipGetErrorString(e != hipSuccess ? e : s));
    // no poison: the trajectory itself is sound
    for (size_t b = 0; b < h->B; ++b)
        if (range[b] != 0)
            return fail(h, LJMD_ERR_RANGE, "%s: replica %zu: a pair's or a particle's %s terms were not finite or "
                                           "|term| >= 2^40 and entered as 0; the flag stays until ljmd_batch_%s_reset", who, b,
                        d.acc.name, d.acc.tag);
    if (n_snapshots) *n_snapshots = q.count;
    return LJMD_OK;
}

int series_read_words(ljmd_batch *h, const BatchSeriesDesc &d, bool want, std::vector<int64_t> *w, int64_t *n_snapshots,
                      const char *who)
{
    LJMD_TRY(enter(h, who, d.need));
    if (want) LJMD_TRY(host_alloc(h, who, [&] { w->resize((size_t)(h->*d.series).count * row_words(h, d)); }));
    return series_fetch(h, d, want ? w->data() : nullptr, n_snapshots, who);
}

int series_configure(ljmd_batch *h, const BatchSeriesDesc &d, int32_t max_snapshots, int32_t every, const char *who)
{
    LJMD_TRY(enter(h, who, 0));
    BatchSeries *q = &(h->*d.series);
    if (max_snapshots < 0 || max_snapshots > d.max_snapshots)
        return fail(h, LJMD_ERR_INVALID_ARG, "%s: max_snapshots = %d outside 1..%d (0 switches the %s off)", who, max_snapshots,
                    d.max_snapshots, d.acc.name);
    if (every < 0) return fail(h, LJMD_ERR_INVALID_ARG, "%s: every must be >= 0", who);
    LJMD_HIP(h, hipSetDevice(h->device));
    series_release(h, d);
    if (max_snapshots == 0) return LJMD_OK;
    const size_t wbytes = (size_t)max_snapshots * row_words(h, d) * sizeof(uint64_t), fbytes = h->B * sizeof(int32_t);
    const std::string what = std::string("the ") + d.acc.name + " series";
    auto body = [&]() -> int {
        LJMD_TRY(device_alloc(h, &q->d_words, wbytes, who, what.c_str()));
        LJMD_TRY(device_alloc(h, &q->d_range, fbytes, who, "range words"));
        LJMD_HIP(h, hipMemsetAsync(q->d_words, 0, wbytes, h->stream));
        LJMD_HIP(h, hipMemsetAsync(q->d_range, 0, fbytes, h->stream));
        return LJMD_OK;                // no wait: nothing here is read from host memory
    };
    const int rc_ = body();
    if (rc_ != LJMD_OK) {
        (void)hipGetLastError();       // a failed hipMalloc is otherwise what the next launch returns (dispatch_class)
        series_release(h, d);
        return rc_;
    }
    q->max_snapshots = max_snapshots;
    q->every = every;
    q->acc = d.acc;
    q->acc.every = every;
    q->release = d.release;
    return LJMD_OK;
}

int series_accumulate(ljmd_batch *h, const BatchSeriesDesc &d, const char *who)
{
    LJMD_TRY(enter(h, who, d.need | kNeedState | kNeedSound | kNeedDevice));
    LJMD_TRY(series_room(h, d, 1, who));
    return accumulate_now(h, (h->*d.series).acc, who);
}

int series_reset(ljmd_batch *h, const BatchSeriesDesc &d, const char *who)
{
    LJMD_TRY(enter(h, who, d.need | kNeedDevice));
    BatchSeries *q = &(h->*d.series);
    LJMD_HIP(h, hipMemsetAsync(q->d_words, 0, (size_t)q->max_snapshots * row_words(h, d) * sizeof(uint64_t), h->stream));
    LJMD_HIP(h, hipMemsetAsync(q->d_range, 0, h->B * sizeof(int32_t), h->stream));
    q->count = 0;
    return LJMD_OK;
}

}  // namespace ljmdb
