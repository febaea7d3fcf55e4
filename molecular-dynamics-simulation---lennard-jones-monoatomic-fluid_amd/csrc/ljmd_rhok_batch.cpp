// ljmd_rhok_batch.cpp -- host side of the batch engine's density modes (include/ljmd.h: ljmd_batch_rhok_*; kernel:
// ljmd_batch_rhok.hip): guards, buffers, the one launch per group and snapshot, reads and resets, and the entry through
// which the step loop of ljmd_batch.cpp takes its snapshots.  A small core of its own on the helpers of ljmd_batch_host.h
// beside the series core (ljmd_batch_series.cpp): a snapshot here has a run-time width of 6 n_modes words per replica, a
// mode list on the device and no pair part -- no rdf_chunk split, no pair-range message -- so that BatchSeriesDesc would
// share little more than the guards.
// The file name does not match ljmd_batch*.cpp on purpose, as ljmd_vanhove_batch.cpp's: the host transcripts of the batch
// engine (tests/batch_trace/Makefile and its like) link every such file with launchers of their own and have none for
// this kernel.  So ljmd_batch.cpp references no symbol of this file: ljmd_batch_rhok_configure leaves the accumulator and
// the release in the handle (BatchRhok), which is how the step loop and ljmd_batch_destroy reach them.  The conversion to
// doubles is ljmdc::rhok_doubles (ljmd_rhok.h), the one of ljmd_rhok_read.
#include "ljmd_batch_host.h"
#include "ljmd_batch_rhok.h"

using namespace ljmdb;

static_assert(kBatchRhokMaxSnapshots == LJMD_BATCH_RHOK_MAX_SNAPSHOTS && kBatchRhokMaxEntries == LJMD_BATCH_RHOK_MAX_ENTRIES &&
                  kBatchRhokMaxN == LJMD_BATCH_MAX_N, "LJMD_BATCH_RHOK_* out of sync with include/ljmd.h");
static_assert(ljmdc::kRhokMaxModes == LJMD_RHOK_MAX_MODES && ljmdc::kRhokMaxIndex == LJMD_RHOK_MAX_INDEX,
              "the mode rules are those of ljmd_rhok_configure");

namespace {

size_t row_words(const ljmd_batch *h) { return h->B * (size_t)h->rhok.n_modes * kBatchRhokRowWords; }

// the launch of group g on stream s for snapshot k of a call: row count + k of the series, every replica of the group
int rhok_enqueue(ljmd_batch *h, const BatchGroup &g, hipStream_t s, int k, int32_t *count, const char *who)
{
    const BatchRhok &q = h->rhok;
    BatchRhokArgs a{};
    a.r = plane(h, LJMD_R, 0);
    a.rep = h->d_table;
    a.modes = q.d_modes;
    a.words = q.d_words;
    a.range = q.d_range;
    a.plane = h->total;
    a.B = h->B;
    a.row = q.count + k;
    a.rows = q.max_snapshots;
    a.g0 = (int)g.first;
    a.n_modes = q.n_modes;
    const hipError_t e = launch_batch_rhok(a, (int)g.count, q.waves, s);
    ++*count;
    if (e != hipSuccess)
        return poison(h, LJMD_ERR_HIP, "%s: density modes launch failed: %s; the handle is poisoned until ljmd_batch_set_state",
                      who, hipGetErrorString(e));
    return LJMD_OK;
}

int rhok_room(ljmd_batch *h, int snapshots, const char *who)
{
    const BatchRhok &q = h->rhok;
    if (q.count + snapshots <= q.max_snapshots) return LJMD_OK;
    return fail(h, LJMD_ERR_STATE, "%s: the density modes series is full: %lld of %d snapshots taken, %d more do not fit "
                                   "(read it, then ljmd_batch_rhok_reset)", who, (long long)q.count, q.max_snapshots, snapshots);
}

// releases the buffers after what may still use them and switches the feature off
void rhok_release(ljmd_batch *h)
{
    BatchRhok *q = &h->rhok;
    if (h->stream && (q->d_words || q->d_modes || q->d_range)) (void)hipStreamSynchronize(h->stream);
    if (q->d_words) (void)hipFree(q->d_words);
    if (q->d_modes) (void)hipFree(q->d_modes);
    if (q->d_range) (void)hipFree(q->d_range);
    for (hipEvent_t e : q->ev)
        if (e) (void)hipEventDestroy(e);
    *q = {};
}

const BatchAccumulator kAcc = {0, "density modes", "rhok", rhok_enqueue,
                               [](ljmd_batch *h, int snapshots) { h->rhok.count += snapshots; }, rhok_room};

// the guards (a poisoned handle may still be read), the series so far in words -- waits for the device; a set range word
// fails the call and names the lowest such replica
int rhok_fetch(ljmd_batch *h, int64_t *words, int64_t *n_snapshots, const char *who)
{
    LJMD_TRY(enter(h, who, kNeedRhok | kNeedDevice));
    const BatchRhok &q = h->rhok;
    std::vector<int32_t> range;
    LJMD_TRY(host_alloc(h, who, [&] { range.resize(h->B); }));
    hipError_t e = hipMemcpyAsync(range.data(), q.d_range, h->B * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess && words && q.count > 0)
        e = hipMemcpyAsync(words, q.d_words, (size_t)q.count * row_words(h) * sizeof(uint64_t), hipMemcpyDeviceToHost,
                           h->stream);
    const hipError_t s = hipStreamSynchronize(h->stream);
    if (e != hipSuccess || s != hipSuccess)
        return poison(h, LJMD_ERR_HIP, "%s: kernel or copy failed: %s; the handle is poisoned until ljmd_batch_set_state",
                      who, hipGetErrorString(e != hipSuccess ? e : s));
    // no poison: the trajectory itself is sound
    for (size_t b = 0; b < h->B; ++b)
        if (range[b] != 0)
            return fail(h, LJMD_ERR_RANGE, "%s: replica %zu: a particle's density mode terms were not finite (a coordinate "
                                           "or the box length is not) and entered as 0; the flag stays until "
                                           "ljmd_batch_rhok_reset", who, b);
    if (n_snapshots) *n_snapshots = q.count;
    return LJMD_OK;
}

}  // namespace

extern "C" {

int ljmd_batch_rhok_configure(ljmd_batch_t *h, int32_t n_modes, const int32_t *modes, int32_t max_snapshots, int32_t every)
{
    static const char *who = "ljmd_batch_rhok_configure";
    LJMD_TRY(enter(h, who, 0));
    BatchRhok *q = &h->rhok;
    if (max_snapshots < 0 || max_snapshots > kBatchRhokMaxSnapshots)
        return fail(h, LJMD_ERR_INVALID_ARG, "%s: max_snapshots = %d outside 1..%d (0 switches the density modes off)", who,
                    max_snapshots, kBatchRhokMaxSnapshots);
    if (every < 0) return fail(h, LJMD_ERR_INVALID_ARG, "%s: every must be >= 0", who);
    if (max_snapshots > 0) {
        if (n_modes < 1 || n_modes > ljmdc::kRhokMaxModes)
            return fail(h, LJMD_ERR_INVALID_ARG, "%s: n_modes = %d outside 1..%d", who, n_modes, ljmdc::kRhokMaxModes);
        if (!modes) return fail(h, LJMD_ERR_INVALID_ARG, "%s: modes is NULL", who);
        for (int m = 0; m < n_modes; ++m)
            for (int a = 0; a < 3; ++a)
                if (modes[3 * m + a] < -ljmdc::kRhokMaxIndex || modes[3 * m + a] > ljmdc::kRhokMaxIndex)
                    return fail(h, LJMD_ERR_INVALID_ARG, "%s: mode %d = (%d, %d, %d): an index outside -%d..%d", who, m,
                                modes[3 * m], modes[3 * m + 1], modes[3 * m + 2], ljmdc::kRhokMaxIndex, ljmdc::kRhokMaxIndex);
        const long long entries = (long long)max_snapshots * (long long)h->B * n_modes;
        if (entries > kBatchRhokMaxEntries)
            return fail(h, LJMD_ERR_INVALID_ARG, "%s: max_snapshots * B * n_modes = %lld above %d", who, entries,
                        kBatchRhokMaxEntries);
    }
    LJMD_HIP(h, hipSetDevice(h->device));
    rhok_release(h);
    if (max_snapshots == 0) return LJMD_OK;
    const size_t wbytes = (size_t)max_snapshots * h->B * (size_t)n_modes * kBatchRhokRowWords * sizeof(uint64_t);
    const size_t mbytes = (size_t)n_modes * 3 * sizeof(int32_t), fbytes = h->B * sizeof(int32_t);
    auto body = [&]() -> int {
        LJMD_TRY(device_alloc(h, &q->d_words, wbytes, who, "the density modes series"));
        LJMD_TRY(device_alloc(h, &q->d_modes, mbytes, who, "the mode list"));
        LJMD_TRY(device_alloc(h, &q->d_range, fbytes, who, "range words"));
        for (hipEvent_t &e : q->ev) LJMD_HIP(h, hipEventCreate(&e));
        LJMD_HIP(h, hipMemsetAsync(q->d_words, 0, wbytes, h->stream));
        LJMD_HIP(h, hipMemsetAsync(q->d_range, 0, fbytes, h->stream));
        LJMD_HIP(h, hipMemcpyAsync(q->d_modes, modes, mbytes, hipMemcpyHostToDevice, h->stream));
        LJMD_HIP(h, hipStreamSynchronize(h->stream));       // the caller's list is free again
        return LJMD_OK;
    };
    const int rc_ = body();
    if (rc_ != LJMD_OK) {
        (void)hipGetLastError();       // a failed hipMalloc is otherwise what the next launch returns
        rhok_release(h);
        return rc_;
    }
    const int waves = ljmdh::read_knobs().batch_rhok_waves;
    q->waves = (waves == 2 || waves == 4 || waves == 8) ? waves : kBatchRhokWaves;
    q->max_snapshots = max_snapshots;
    q->n_modes = n_modes;
    q->every = every;
    q->acc = kAcc;
    q->acc.every = every;
    q->release = rhok_release;
    return LJMD_OK;
}

int ljmd_batch_rhok_accumulate(ljmd_batch_t *h)
{
    static const char *who = "ljmd_batch_rhok_accumulate";
    LJMD_TRY(enter(h, who, kNeedRhok | kNeedState | kNeedSound | kNeedDevice));
    LJMD_TRY(rhok_room(h, 1, who));
    h->rhok.timed = false;
    LJMD_HIP(h, hipEventRecord(h->rhok.ev[0], h->stream));
    LJMD_TRY(accumulate_now(h, h->rhok.acc, who));
    LJMD_HIP(h, hipEventRecord(h->rhok.ev[1], h->stream));
    h->rhok.timed = true;
    return LJMD_OK;
}

int ljmd_batch_rhok_read_exact(ljmd_batch_t *h, int64_t *words, int64_t *n_snapshots)
{
    static const char *who = "ljmd_batch_rhok_read_exact";
    return rhok_fetch(h, words, n_snapshots, who);
}

int ljmd_batch_rhok_read(ljmd_batch_t *h, double *rho, int64_t *n_snapshots)
{
    static const char *who = "ljmd_batch_rhok_read";
    LJMD_TRY(enter(h, who, kNeedRhok));
    std::vector<int64_t> w;
    if (rho) LJMD_TRY(host_alloc(h, who, [&] { w.resize((size_t)h->rhok.count * row_words(h)); }));
    LJMD_TRY(rhok_fetch(h, rho ? w.data() : nullptr, n_snapshots, who));
    if (rho) ljmdc::rhok_doubles(w.data(), w.size() / 3, rho);
    return LJMD_OK;
}

int ljmd_batch_rhok_reset(ljmd_batch_t *h)
{
    static const char *who = "ljmd_batch_rhok_reset";
    LJMD_TRY(enter(h, who, kNeedRhok | kNeedDevice));
    BatchRhok *q = &h->rhok;
    LJMD_HIP(h, hipMemsetAsync(q->d_words, 0, (size_t)q->max_snapshots * row_words(h) * sizeof(uint64_t), h->stream));
    LJMD_HIP(h, hipMemsetAsync(q->d_range, 0, h->B * sizeof(int32_t), h->stream));
    q->count = 0;
    return LJMD_OK;
}

int ljmd_batch_rhok_profile_read(ljmd_batch_t *h, double *kernel_ms)
{
    static const char *who = "ljmd_batch_rhok_profile_read";
    LJMD_TRY(enter(h, who, kNeedRhok | kNeedDevice));
    float ms = 0.0f;
    if (h->rhok.timed) {
        LJMD_HIP(h, hipEventSynchronize(h->rhok.ev[1]));
        LJMD_HIP(h, hipEventElapsedTime(&ms, h->rhok.ev[0], h->rhok.ev[1]));
    }
    if (kernel_ms) *kernel_ms = (double)ms;
    return LJMD_OK;
}

}  // extern "C"
