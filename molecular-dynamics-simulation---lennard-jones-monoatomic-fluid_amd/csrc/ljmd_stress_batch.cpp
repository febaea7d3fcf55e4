// ljmd_stress_batch.cpp -- host side of the batch engine's pressure tensor (include/ljmd.h: ljmd_batch_stress_*; kernel:
// ljmd_batch_stress.hip): configure / accumulate / read / reset of the series, and the entry through which the step loop
// of ljmd_batch.cpp takes its snapshots.
// The file name does not match ljmd_batch*.cpp on purpose, as ljmd_prepare.cpp's: the host transcripts of the batch engine
// (tests/batch_trace/Makefile, tests/prepare_host/Makefile) link every such file with launchers of their own and have
// none for this kernel.  So ljmd_batch.cpp references no symbol of this file: ljmd_batch_stress_configure leaves the
// accumulator and the release in the handle (BatchStress), which is how the step loop and ljmd_batch_destroy reach them.
#include "ljmd_batch_host.h"
#include "ljmd_batch_stress.h"
#include "ljmd_stress.h"

using namespace ljmdb;

static_assert(kBatchStressMaxSnapshots == LJMD_BATCH_STRESS_MAX_SNAPSHOTS, "series limit out of sync with include/ljmd.h");
static_assert(kBatchStressWords == ljmds::kStressWords, "one snapshot of one replica is a snapshot of ljmd_stress_*");

namespace {

size_t row_words(const ljmd_batch *h) { return h->B * (size_t)kBatchStressWords; }

// the launches of group g on stream s for snapshot k of a call: row count + k of the series, chunks of at most rdf_chunk
// replicas (launch_shape's pair bound of the fp64 mode, one step)
int enqueue_stress(ljmd_batch *h, const BatchGroup &g, hipStream_t s, int k, int32_t *count, const char *who)
{
    BatchStressArgs sa{};
    sa.state = h->d_state;
    sa.words = h->stress.d_words;
    sa.range = h->stress.d_range;
    sa.rep = h->d_table;
    sa.plane = h->total;
    sa.B = h->B;
    sa.row = h->stress.count + k;
    sa.rows = h->stress.max_snapshots;
    for (size_t c0 = 0; c0 < g.count; c0 += g.rdf_chunk) {
        sa.g0 = (int)(g.first + c0);
        const hipError_t e = launch_batch_stress(sa, g.n_max, (int)std::min(g.rdf_chunk, g.count - c0), s);
        ++*count;
        if (e != hipSuccess)
            return poison(h, LJMD_ERR_HIP, "%s: pressure tensor launch failed: %s; the handle is poisoned until "
                                           "ljmd_batch_set_state", who, hipGetErrorString(e));
    }
    return LJMD_OK;
}

void stress_ran(ljmd_batch *h, int snapshots) { h->stress.count += snapshots; }

int stress_room(ljmd_batch *h, int snapshots, const char *who)
{
    if (h->stress.count + snapshots <= h->stress.max_snapshots) return LJMD_OK;
    return fail(h, LJMD_ERR_STATE, "%s: the pressure tensor series is full: %lld of %d snapshots taken, %d more do not fit "
                                   "(read it, then ljmd_batch_stress_reset)", who, (long long)h->stress.count,
                h->stress.max_snapshots, snapshots);
}

// releases the series after what may still use it and switches the feature off
void stress_release(ljmd_batch *h)
{
    if (h->stream && (h->stress.d_words || h->stress.d_range)) (void)hipStreamSynchronize(h->stream);
    if (h->stress.d_words) (void)hipFree(h->stress.d_words);
    if (h->stress.d_range) (void)hipFree(h->stress.d_range);
    h->stress = {};
}

// what ljmd_batch_stress_read and ljmd_batch_stress_read_exact share: the guards (a poisoned handle may still be read),
// the series so far in words -- waits for the device; a set range word fails the call and names the lowest such replica
int stress_fetch(ljmd_batch *h, int64_t *words, int64_t *n_snapshots, const char *who)
{
    LJMD_TRY(enter(h, who, kNeedStress | kNeedDevice));
    std::vector<int32_t> range;
    LJMD_TRY(host_alloc(h, who, [&] { range.resize(h->B); }));
    hipError_t e = hipMemcpyAsync(range.data(), h->stress.d_range, h->B * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess && words && h->stress.count > 0)
        e = hipMemcpyAsync(words, h->stress.d_words, (size_t)h->stress.count * row_words(h) * sizeof(uint64_t),
                           hipMemcpyDeviceToHost, h->stream);
    const hipError_t s = hipStreamSynchronize(h->stream);
    if (e != hipSuccess || s != hipSuccess)
        return poison(h, LJMD_ERR_HIP, "%s: kernel or copy failed: %s; the handle is poisoned until ljmd_batch_set_state",
                      who, hipGetErrorString(e != hipSuccess ? e : s));
    // no poison: the trajectory itself is sound
    for (size_t b = 0; b < h->B; ++b)
        if (range[b] != 0)
            return fail(h, LJMD_ERR_RANGE, "%s: replica %zu: a pair's or a particle's pressure tensor terms were not finite "
                                           "or |term| >= 2^40 and entered as 0; the flag stays until "
                                           "ljmd_batch_stress_reset", who, b);
    if (n_snapshots) *n_snapshots = h->stress.count;
    return LJMD_OK;
}

}  // namespace

extern "C" {

int ljmd_batch_stress_configure(ljmd_batch_t *h, int32_t max_snapshots, int32_t every)
{
    static const char *who = "ljmd_batch_stress_configure";
    LJMD_TRY(enter(h, who, 0));
    if (max_snapshots < 0 || max_snapshots > kBatchStressMaxSnapshots)
        return fail(h, LJMD_ERR_INVALID_ARG, "%s: max_snapshots = %d outside 1..%d (0 switches the pressure tensor off)", who,
                     max_snapshots, kBatchStressMaxSnapshots);
    if (every < 0) return fail(h, LJMD_ERR_INVALID_ARG, "%s: every must be >= 0", who);
    LJMD_HIP(h, hipSetDevice(h->device));
    stress_release(h);
    if (max_snapshots == 0) return LJMD_OK;
    const size_t wbytes = (size_t)max_snapshots * row_words(h) * sizeof(uint64_t), fbytes = h->B * sizeof(int32_t);
    auto body = [&]() -> int {
        LJMD_TRY(device_alloc(h, &h->stress.d_words, wbytes, who, "the pressure tensor series"));
        LJMD_TRY(device_alloc(h, &h->stress.d_range, fbytes, who, "range words"));
        LJMD_HIP(h, hipMemsetAsync(h->stress.d_words, 0, wbytes, h->stream));
        LJMD_HIP(h, hipMemsetAsync(h->stress.d_range, 0, fbytes, h->stream));
        return LJMD_OK;                // no wait: nothing here is read from host memory
    };
    const int rc_ = body();
    if (rc_ != LJMD_OK) {
        (void)hipGetLastError();       // a failed hipMalloc is otherwise what the next launch returns (dispatch_class)
        stress_release(h);
        return rc_;
    }
    h->stress.max_snapshots = max_snapshots;
    h->stress.every = every;
    h->stress.acc = {every, "pressure tensor", "stress", enqueue_stress, stress_ran, stress_room};
    h->stress.release = stress_release;
    return LJMD_OK;
}

int ljmd_batch_stress_accumulate(ljmd_batch_t *h)
{
    static const char *who = "ljmd_batch_stress_accumulate";
    LJMD_TRY(enter(h, who, kNeedStress | kNeedState | kNeedSound | kNeedDevice));
    LJMD_TRY(stress_room(h, 1, who));
    return accumulate_now(h, h->stress.acc, who);
}

int ljmd_batch_stress_read_exact(ljmd_batch_t *h, int64_t *words, int64_t *n_snapshots)
{
    return stress_fetch(h, words, n_snapshots, "ljmd_batch_stress_read_exact");
}

int ljmd_batch_stress_read(ljmd_batch_t *h, double *p, int64_t *n_snapshots)
{
    static const char *who = "ljmd_batch_stress_read";
    LJMD_TRY(enter(h, who, kNeedStress));
    std::vector<int64_t> w;
    if (p) LJMD_TRY(host_alloc(h, who, [&] { w.resize((size_t)h->stress.count * row_words(h)); }));
    LJMD_TRY(stress_fetch(h, p ? w.data() : nullptr, n_snapshots, who));
    for (size_t s = 0; p && s < (size_t)h->stress.count; ++s)
        for (size_t b = 0; b < h->B; ++b) {
            const size_t o = s * h->B + b;
            ljmds::stress_doubles(w.data() + o * kBatchStressWords, h->rep[b].L, p + o * ljmds::kStressComponents);
        }
    return LJMD_OK;
}

int ljmd_batch_stress_reset(ljmd_batch_t *h)
{
    static const char *who = "ljmd_batch_stress_reset";
    LJMD_TRY(enter(h, who, kNeedStress | kNeedDevice));
    LJMD_HIP(h, hipMemsetAsync(h->stress.d_words, 0, (size_t)h->stress.max_snapshots * row_words(h) * sizeof(uint64_t),
                                h->stream));
    LJMD_HIP(h, hipMemsetAsync(h->stress.d_range, 0, h->B * sizeof(int32_t), h->stream));
    h->stress.count = 0;
    return LJMD_OK;
}

}  // extern "C"
