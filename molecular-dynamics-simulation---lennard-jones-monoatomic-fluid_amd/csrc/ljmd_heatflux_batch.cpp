// ljmd_heatflux_batch.cpp -- host side of the batch engine's heat flux (include/ljmd.h: ljmd_batch_heatflux_*; kernel:
// ljmd_batch_heatflux.hip): its descriptor for the series core (ljmd_batch_series.cpp), the C entry points, the
// conversion to doubles, and the entry through which the step loop of ljmd_batch.cpp takes its snapshots.
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

// the entries of the step loop and of ljmd_batch_destroy pass the descriptor on: that is all they know of this file
const BatchSeriesDesc kDesc = {
    &ljmd_batch::heatflux,
    {0, "heat flux", "heatflux",
     [](ljmd_batch *h, const BatchGroup &g, hipStream_t s, int k, int32_t *count, const char *who) {
         return series_enqueue(h, kDesc, g, s, k, count, who);
     },
     [](ljmd_batch *h, int snapshots) { h->heatflux.count += snapshots; },
     [](ljmd_batch *h, int snapshots, const char *who) { return series_room(h, kDesc, snapshots, who); }},
    [](ljmd_batch *h) { series_release(h, kDesc); },
    kBatchHeatfluxWords, kBatchHeatfluxMaxSnapshots, kNeedHeatflux, launch_batch_heatflux};

}  // namespace

extern "C" {

int ljmd_batch_heatflux_configure(ljmd_batch_t *h, int32_t max_snapshots, int32_t every)
{
    static const char *who = "ljmd_batch_heatflux_configure";
    return series_configure(h, kDesc, max_snapshots, every, who);
}

int ljmd_batch_heatflux_accumulate(ljmd_batch_t *h)
{
    static const char *who = "ljmd_batch_heatflux_accumulate";
    return series_accumulate(h, kDesc, who);
}

int ljmd_batch_heatflux_read_exact(ljmd_batch_t *h, int64_t *words, int64_t *n_snapshots)
{
    static const char *who = "ljmd_batch_heatflux_read_exact";
    return series_fetch(h, kDesc, words, n_snapshots, who);
}

int ljmd_batch_heatflux_read(ljmd_batch_t *h, double *j, double *parts, int64_t *n_snapshots)
{
    static const char *who = "ljmd_batch_heatflux_read";
    const bool want = j || parts;
    std::vector<int64_t> w;
    LJMD_TRY(series_read_words(h, kDesc, want, &w, n_snapshots, who));
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
    return series_reset(h, kDesc, who);
}

}  // extern "C"
