// ljmd_stress_batch.cpp -- host side of the batch engine's pressure tensor (include/ljmd.h: ljmd_batch_stress_*; kernel:
// ljmd_batch_stress.hip): its descriptor for the series core (ljmd_batch_series.cpp), the C entry points, the conversion
// to doubles, and the entry through which the step loop of ljmd_batch.cpp takes its snapshots.
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

// the entries of the step loop and of ljmd_batch_destroy pass the descriptor on: that is all they know of this file
const BatchSeriesDesc kDesc = {
    &ljmd_batch::stress,
    {0, "pressure tensor", "stress",
     [](ljmd_batch *h, const BatchGroup &g, hipStream_t s, int k, int32_t *count, const char *who) {
         return series_enqueue(h, kDesc, g, s, k, count, who);
     },
     [](ljmd_batch *h, int snapshots) { h->stress.count += snapshots; },
     [](ljmd_batch *h, int snapshots, const char *who) { return series_room(h, kDesc, snapshots, who); }},
    [](ljmd_batch *h) { series_release(h, kDesc); },
    kBatchStressWords, kBatchStressMaxSnapshots, kNeedStress, launch_batch_stress};

}  // namespace

extern "C" {

int ljmd_batch_stress_configure(ljmd_batch_t *h, int32_t max_snapshots, int32_t every)
{
    static const char *who = "ljmd_batch_stress_configure";
    return series_configure(h, kDesc, max_snapshots, every, who);
}

int ljmd_batch_stress_accumulate(ljmd_batch_t *h)
{
    static const char *who = "ljmd_batch_stress_accumulate";
    return series_accumulate(h, kDesc, who);
}

int ljmd_batch_stress_read_exact(ljmd_batch_t *h, int64_t *words, int64_t *n_snapshots)
{
    static const char *who = "ljmd_batch_stress_read_exact";
    return series_fetch(h, kDesc, words, n_snapshots, who);
}

int ljmd_batch_stress_read(ljmd_batch_t *h, double *p, int64_t *n_snapshots)
{
    static const char *who = "ljmd_batch_stress_read";
    std::vector<int64_t> w;
    LJMD_TRY(series_read_words(h, kDesc, p != nullptr, &w, n_snapshots, who));
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
    return series_reset(h, kDesc, who);
}

}  // extern "C"
