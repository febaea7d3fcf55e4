// ljmd_heatflux_batch.cpp -- host side of the batch engine's heat flux (include/ljmd.h: ljmd_batch_heatflux_*; kernel:
// ljmd_batch_heatflux.hip): configure / accumulate / read / reset of the series, and the entry through which the step
// loop of ljmd_batch.cpp takes its snapshots.
// The file name does not match ljmd_batch*.cpp on purpose, as ljmd_stress_batch.cpp's: the host transcripts of the batch
// engine (tests/batch_trace/Makefile, tests/prepare_host/Makefile, tests/batch_stress_host/Makefile) link every such file
// with launchers of their own and have none for this kernel.  So ljmd_batch.cpp references no symbol of this file:
// ljmd_batch_heatflux_configure leaves the accumulator and the release in the handle (BatchHeatflux), which is how the
// step loop and ljmd_batch_destroy reach them.  The conversion to doubles is the inline copy of ljmd_heatflux.h: nothing
// of ljmd_heatflux.cpp is needed.
#include "ljmd_batch_heatflux.h"
#include "ljmd_batch_host.h"
#include "ljmd_heatflux.h"

using namespace ljmdb;

static_assert(kBatchHeatfluxMaxSnapshots == LJMD_BATCH_HEATFLUX_MAX_SNAPSHOTS, "series limit out of sync with include/ljmd.h");
static_assert(kBatchHeatfluxWords == ljmdq::kHeatfluxWords, "one snapshot of one replica is a snapshot of ljmd_heatflux_*");

namespace {

size_t row_words(const ljmd_batch *h) { return h->B * (size_t)kBatchHeatfluxWords; }

// the launches of group g on stream s for snapshot k of a call: row count + k of the series, chunks of at most rdf_chunk
// replicas (launch_shape's pair bound of the fp64 mode, one step)
int enqueue_heatflux(ljmd_batch *h, const BatchGroup &g, hipStream_t s, int k, int32_t *count, const char *who)
{
    BatchHeatfluxArgs ha{};
    ha.state = h->d_state;
    ha.words = h->heatflux.d_words;
    ha.range = h->heatflux.d_range;
    ha.rep = h->d_table;
    ha.plane = h->total;
    ha.B = h->B;
    ha.row = h->heatflux.count + k;
    ha.rows = h->heatflux.max_snapshots;
    for (size_t c0 = 0; c0 < g.count; c0 += g.rdf_chunk) {
        ha.g0 = (int)(g.first + c0);
        const hipError_t e = launch_batch_heatflux(ha, g.n_max, (int)std::min(g.rdf_chunk, g.count - c0), s);
        ++*count;
        if (e != hipSuccess)
            return poison(h, LJMD_ERR_HIP, "%s: heat flux launch failed: %s; the handle is poisoned until "
                                           "ljmd_batch_set_state", who, hipGetErrorString(e));
    }
    return LJMD_OK;
}

void heatflux_ran(ljmd_batch *h, int snapshots) { h->heatflux.count += snapshots; }

int heatflux_room(ljmd_batch *h, int snapshots, const char *who)
{
    if (h->heatflux.count + snapshots <= h->heatflux.max_snapshots) return LJMD_OK;
    return fail(h, LJMD_ERR_STATE, "%s: the heat flux series is full: %lld of %d snapshots taken, %d more do not fit "
                                   "(read it, then ljmd_batch_heatflux_reset)", who, (long long)h->heatflux.count,
                h->heatflux.max_snapshots, snapshots);
}

// releases the series after what may still use it and switches the feature off
void heatflux_release(ljmd_batch *h)
{
    if (h->stream && (h->heatflux.d_words || h->heatflux.d_range)) (void)hipStreamSynchronize(h->stream);
    if (h->heatflux.d_words) (void)hipFree(h->heatflux.d_words);
    if (h->heatflux.d_range) (void)hipFree(h->heatflux.d_range);
    h->heatflux = {};
}

// what ljmd_batch_heatflux_read and ljmd_batch_heatflux_read_exact share: the guards (a poisoned handle may still be
// read), the series so far in words -- waits for the device; a set range word fails the call and names the lowest such
// replica
int heatflux_fetch(ljmd_batch *h, int64_t *words, int64_t *n_snapshots, const char *who)
{
    LJMD_TRY(enter(h, who, kNeedHeatflux | kNeedDevice));
    std::vector<int32_t> range;
    LJMD_TRY(host_alloc(h, who, [&] { range.resize(h->B); }));
    hipError_t e = hipMemcpyAsync(range.data(), h->heatflux.d_range, h->B * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess && words && h->heatflux.count > 0)
        e = hipMemcpyAsync(words, h->heatflux.d_words, (size_t)h->heatflux.count * row_words(h) * sizeof(uint64_t),
                           hipMemcpyDeviceToHost, h->stream);
    const hipError_t s = hipStreamSynchronize(h->stream);
    if (e != hipSuccess || s != hipSuccess)
        return poison(h, LJMD_ERR_HIP, "%s: kernel or copy failed: %s; the handle is poisoned until ljmd_batch_set_state",
                      who, hipGetErrorString(e != hipSuccess ? e : s));
    // no poison: the trajectory itself is sound
    for (size_t b = 0; b < h->B; ++b)
        if (range[b] != 0)
            return fail(h, LJMD_ERR_RANGE, "%s: replica %zu: a pair's or a particle's heat flux terms were not finite or "
                                           "|term| >= 2^40 and entered as 0; the flag stays until "
                                           "ljmd_batch_heatflux_reset", who, b);
    if (n_snapshots) *n_snapshots = h->heatflux.count;
    return LJMD_OK;
}

}  // namespace

extern "C" {

int ljmd_batch_heatflux_configure(ljmd_batch_t *h, int32_t max_snapshots, int32_t every)
{
    static const char *who = "ljmd_batch_heatflux_configure";
    LJMD_TRY(enter(h, who, 0));
    if (max_snapshots < 0 || max_snapshots > kBatchHeatfluxMaxSnapshots)
        return fail(h, LJMD_ERR_INVALID_ARG, "%s: max_snapshots = %d outside 1..%d (0 switches the heat flux off)", who,
                     max_snapshots, kBatchHeatfluxMaxSnapshots);
    if (every < 0) return fail(h, LJMD_ERR_INVALID_ARG, "%s: every must be >= 0", who);
    LJMD_HIP(h, hipSetDevice(h->device));
    heatflux_release(h);
    if (max_snapshots == 0) return LJMD_OK;
    const size_t wbytes = (size_t)max_snapshots * row_words(h) * sizeof(uint64_t), fbytes = h->B * sizeof(int32_t);
    auto body = [&]() -> int {
        LJMD_TRY(device_alloc(h, &h->heatflux.d_words, wbytes, who, "the heat flux series"));
        LJMD_TRY(device_alloc(h, &h->heatflux.d_range, fbytes, who, "range words"));
        LJMD_HIP(h, hipMemsetAsync(h->heatflux.d_words, 0, wbytes, h->stream));
        LJMD_HIP(h, hipMemsetAsync(h->heatflux.d_range, 0, fbytes, h->stream));
        return LJMD_OK;                // no wait: nothing here is read from host memory
    };
    const int rc_ = body();
    if (rc_ != LJMD_OK) {
        (void)hipGetLastError();       // a failed hipMalloc is otherwise what the next launch returns (dispatch_class)
        heatflux_release(h);
        return rc_;
    }
    h->heatflux.max_snapshots = max_snapshots;
    h->heatflux.every = every;
    h->heatflux.acc = {every, "heat flux", "heatflux", enqueue_heatflux, heatflux_ran, heatflux_room};
    h->heatflux.release = heatflux_release;
    return LJMD_OK;
}

int ljmd_batch_heatflux_accumulate(ljmd_batch_t *h)
{
    static const char *who = "ljmd_batch_heatflux_accumulate";
    LJMD_TRY(enter(h, who, kNeedHeatflux | kNeedState | kNeedSound | kNeedDevice));
    LJMD_TRY(heatflux_room(h, 1, who));
    return accumulate_now(h, h->heatflux.acc, who);
}

int ljmd_batch_heatflux_read_exact(ljmd_batch_t *h, int64_t *words, int64_t *n_snapshots)
{
    return heatflux_fetch(h, words, n_snapshots, "ljmd_batch_heatflux_read_exact");
}

int ljmd_batch_heatflux_read(ljmd_batch_t *h, double *j, double *parts, int64_t *n_snapshots)
{
    static const char *who = "ljmd_batch_heatflux_read";
    LJMD_TRY(enter(h, who, kNeedHeatflux));
    const bool want = j || parts;
    std::vector<int64_t> w;
    if (want) LJMD_TRY(host_alloc(h, who, [&] { w.resize((size_t)h->heatflux.count * row_words(h)); }));
    LJMD_TRY(heatflux_fetch(h, want ? w.data() : nullptr, n_snapshots, who));
    for (size_t s = 0; want && s < (size_t)h->heatflux.count; ++s)
        for (size_t b = 0; b < h->B; ++b) {
            const size_t o = s * h->B + b;
            ljmdq::heatflux_doubles(w.data() + o * kBatchHeatfluxWords, h->rep[b].L, j ? j + o * 3 : nullptr,
                                    parts ? parts + o * 9 : nullptr);
        }
    return LJMD_OK;
}

int ljmd_batch_heatflux_reset(ljmd_batch_t *h)
{
    static const char *who = "ljmd_batch_heatflux_reset";
    LJMD_TRY(enter(h, who, kNeedHeatflux | kNeedDevice));
    LJMD_HIP(h, hipMemsetAsync(h->heatflux.d_words, 0, (size_t)h->heatflux.max_snapshots * row_words(h) * sizeof(uint64_t),
                                h->stream));
    LJMD_HIP(h, hipMemsetAsync(h->heatflux.d_range, 0, h->B * sizeof(int32_t), h->stream));
    h->heatflux.count = 0;
    return LJMD_OK;
}

}  // extern "C"
