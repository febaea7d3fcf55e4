// ljmd_vanhove_batch.cpp -- host side of the batch engine's van Hove self-correlation (include/ljmd.h:
// ljmd_batch_vanhove_*; kernel: ljmd_batch_vanhove.hip): its descriptor for the core of the time-origin observables
// (ljmd_batch_origins.cpp), the C entry points, and the bin widths with their guards.
// The file name does not match ljmd_batch*.cpp on purpose, as ljmd_stress_batch.cpp's and ljmd_heatflux_batch.cpp's: the
// host transcripts of the batch engine (tests/batch_trace/Makefile and its like) link every such file with launchers of
// their own and have none for this kernel.  So ljmd_batch.cpp references no symbol of this file:
// ljmd_batch_vanhove_configure leaves the accumulator and the release in the handle (BatchVanhove), which is how the step
// loop and ljmd_batch_destroy reach them.
#include "ljmd_batch_host.h"
#include "ljmd_batch_vanhove.h"

using namespace ljmdb;

static_assert(kBatchVanhoveMaxLag == LJMD_BATCH_VANHOVE_MAX_LAG && kBatchVanhoveMaxOrigins == LJMD_BATCH_VANHOVE_MAX_ORIGINS &&
                  kBatchVanhoveMaxBins == LJMD_BATCH_VANHOVE_MAX_BINS, "van Hove limits out of sync with include/ljmd.h");

namespace {

// a set range word fails a read after the caller's arrays are filled: the overflow column says where the particles went
const BatchOriginDesc kDesc = {
    &ljmd_batch::vanhove, kNeedVanhove, 3, kBatchVanhoveMaxLag, kBatchVanhoveMaxOrigins, kBatchVanhoveMaxBins,
    "the van Hove function", "VANHOVE",
    "a van Hove displacement was not finite or r^4 >= 2^40: it was counted in the overflow column and entered the sums as 0",
    false,
    {0, "van Hove", "vanhove",
     [](ljmd_batch *h, const BatchGroup &g, hipStream_t s, int k, int32_t *count, const char *who) {
         return origins_enqueue(h, kDesc, g, s, k, count, who);
     },
     [](ljmd_batch *h, int snapshots) { origins_ran(h, kDesc, snapshots); }, nullptr},
    [](ljmd_batch *h) { origins_release(h, kDesc); },
    [](const ljmd_batch *h, const BatchOrigins &q, const BatchOriginArgs &a, int n_max, int n_blocks, hipStream_t s) {
        BatchVanhoveArgs v{};
        static_cast<BatchOriginArgs &>(v) = a;
        v.hist = q.d_hist;
        v.dr = q.d_dr;
        v.inv_dr = q.d_dr + h->B;
        v.nbins = q.nbins;
        return launch_batch_vanhove(v, n_max, n_blocks, s);
    }};

}  // namespace

extern "C" {

int ljmd_batch_vanhove_configure(ljmd_batch_t *h, int32_t max_lag, int32_t origin_stride, int32_t nbins, const double *rmax,
                                 int32_t every)
{
    static const char *who = "ljmd_batch_vanhove_configure";
    LJMD_TRY(origins_configure_guards(h, kDesc, max_lag, origin_stride, every, who));
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
    return origins_configure(h, kDesc, max_lag, origin_stride, every, nbins, dr.data(), who);
}

int ljmd_batch_vanhove_accumulate(ljmd_batch_t *h)
{
    static const char *who = "ljmd_batch_vanhove_accumulate";
    return origins_accumulate(h, kDesc, who);
}

int ljmd_batch_vanhove_read(ljmd_batch_t *h, uint64_t *hist, double *r2, double *r4, int64_t *counts, int64_t *n_snapshots)
{
    static const char *who = "ljmd_batch_vanhove_read";
    return origins_read(h, kDesc, hist, r2, r4, counts, n_snapshots, who);
}

int ljmd_batch_vanhove_read_exact(ljmd_batch_t *h, uint64_t *hist, int64_t *words, int64_t *counts, int64_t *n_snapshots)
{
    static const char *who = "ljmd_batch_vanhove_read_exact";
    return origins_read_exact(h, kDesc, hist, words, counts, n_snapshots, who);
}

int ljmd_batch_vanhove_reset(ljmd_batch_t *h)
{
    static const char *who = "ljmd_batch_vanhove_reset";
    return origins_reset(h, kDesc, who);
}

}  // extern "C"
