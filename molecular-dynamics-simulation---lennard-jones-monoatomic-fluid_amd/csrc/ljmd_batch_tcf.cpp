// ljmd_batch_tcf.cpp -- host side of the batch engine's MSD / VACF accumulation (include/ljmd.h: ljmd_batch_tcf_*,
// ljmd_tcf_from_exact; kernel: ljmd_batch_tcf.hip): its descriptor for the core of the time-origin observables
// (ljmd_batch_origins.cpp), the C entry points, and the entries through which the step loop of ljmd_batch.cpp takes its
// snapshots and ljmd_batch_destroy releases it (tcf_accumulator, tcf_release).
#include "ljmd_batch_host.h"
#include "ljmd_tcf_host.h"

using namespace ljmdb;

static_assert(kBatchTcfMaxLag == LJMD_BATCH_TCF_MAX_LAG && kBatchTcfMaxOrigins == LJMD_BATCH_TCF_MAX_ORIGINS,
              "MSD / VACF limits out of sync with include/ljmd.h");

namespace {

// a set range word fails a read before anything is written to the caller's arrays, counts or n_snapshots
const BatchOriginDesc kDesc = {
    &ljmd_batch::tcf, kNeedTcf, 6, kBatchTcfMaxLag, kBatchTcfMaxOrigins, 0, "MSD / VACF", "TCF",
    "an MSD or VACF term was not finite or |term| >= 2^40 and entered as 0", true,
    {0, "MSD / VACF", "tcf",
     [](ljmd_batch *h, const BatchGroup &g, hipStream_t s, int k, int32_t *count, const char *who) {
         return origins_enqueue(h, kDesc, g, s, k, count, who);
     },
     [](ljmd_batch *h, int snapshots) { origins_ran(h, kDesc, snapshots); }, nullptr},
    [](ljmd_batch *h) { origins_release(h, kDesc); },
    [](const ljmd_batch *, const BatchOrigins &, const BatchOriginArgs &a, int n_max, int n_blocks, hipStream_t s) {
        return launch_batch_tcf(a, n_max, n_blocks, s);
    }};

}  // namespace

BatchAccumulator ljmdb::tcf_accumulator(const ljmd_batch *h)
{
    BatchAccumulator a = kDesc.acc;
    a.every = h->tcf.every;
    return a;
}

void ljmdb::tcf_release(ljmd_batch *h) { origins_release(h, kDesc); }

extern "C" {

int ljmd_batch_tcf_configure(ljmd_batch_t *h, int32_t max_lag, int32_t origin_stride, int32_t every)
{
    static const char *who = "ljmd_batch_tcf_configure";
    LJMD_TRY(origins_configure_guards(h, kDesc, max_lag, origin_stride, every, who));
    return origins_configure(h, kDesc, max_lag, origin_stride, every, 0, nullptr, who);
}

int ljmd_batch_tcf_accumulate(ljmd_batch_t *h)
{
    static const char *who = "ljmd_batch_tcf_accumulate";
    return origins_accumulate(h, kDesc, who);
}

int ljmd_tcf_from_exact(const int64_t *words, int32_t n, int64_t count, double *out)
{
    if (!words || !out) return fail(nullptr, LJMD_ERR_INVALID_ARG, "ljmd_tcf_from_exact: NULL argument");
    if (n < 1 || count < 0) return fail(nullptr, LJMD_ERR_INVALID_ARG, "ljmd_tcf_from_exact: n must be >= 1, count >= 0");
    const uint64_t x[3] = {(uint64_t)words[0], (uint64_t)words[1], (uint64_t)words[2]};
    *out = ljmdh::tcf_quotient(x, n, count);
    return LJMD_OK;
}

int ljmd_batch_tcf_read(ljmd_batch_t *h, double *msd, double *vacf, int64_t *counts, int64_t *n_snapshots)
{
    static const char *who = "ljmd_batch_tcf_read";
    return origins_read(h, kDesc, nullptr, msd, vacf, counts, n_snapshots, who);
}

int ljmd_batch_tcf_read_exact(ljmd_batch_t *h, int64_t *words, int64_t *counts, int64_t *n_snapshots)
{
    static const char *who = "ljmd_batch_tcf_read_exact";
    return origins_read_exact(h, kDesc, nullptr, words, counts, n_snapshots, who);
}

int ljmd_batch_tcf_reset(ljmd_batch_t *h)
{
    static const char *who = "ljmd_batch_tcf_reset";
    return origins_reset(h, kDesc, who);
}

}  // extern "C"
