// ljmd_batch_rdf.cpp -- host side of the batch engine's g(r) accumulation (include/ljmd.h: ljmd_batch_rdf_*; kernel:
// ljmd_batch_rdf.hip): configure / accumulate / read / reset, and the entry through which the step loop of
// ljmd_batch.cpp takes its snapshots.
#include "ljmd_batch_host.h"

using namespace ljmdb;

namespace {

// the g(r) launches of group g on stream s: the positions resident now, chunks of at most rdf_chunk replicas
int enqueue_rdf(ljmd_batch *h, const BatchGroup &g, hipStream_t s, int, int32_t *count, const char *who)
{
    BatchRdfArgs ra{};
    ra.r = plane(h, LJMD_R, 0);
    ra.rep = h->d_table;
    ra.rdf = h->rdf.d_table;
    ra.hist = h->rdf.d_hist;
    ra.plane = h->total;
    ra.nbins = h->rdf.nbins;
    for (size_t c0 = 0; c0 < g.count; c0 += g.rdf_chunk) {
        ra.g0 = (int)(g.first + c0);
        const hipError_t e = launch_batch_rdf(ra, g.n_max, (int)std::min(g.rdf_chunk, g.count - c0), s);
        ++*count;
        if (e != hipSuccess)
            return poison(h, LJMD_ERR_HIP, "%s: g(r) launch failed: %s; the handle is poisoned until ljmd_batch_set_state",
                          who, hipGetErrorString(e));
    }
    return LJMD_OK;
}

void rdf_ran(ljmd_batch *h, int snapshots) { h->rdf.snapshots += snapshots; }

}  // namespace

BatchAccumulator ljmdb::rdf_accumulator(const ljmd_batch *h)
{
    return {h->rdf.every, "g(r)", "rdf", enqueue_rdf, rdf_ran};
}

// releases the g(r) buffers after what may still use them
void ljmdb::rdf_release(ljmd_batch *h)
{
    if (h->stream && (h->rdf.d_hist || h->rdf.d_table)) (void)hipStreamSynchronize(h->stream);
    if (h->rdf.d_hist) (void)hipFree(h->rdf.d_hist);
    if (h->rdf.d_table) (void)hipFree(h->rdf.d_table);
    h->rdf = {};
}

extern "C" {

int ljmd_batch_rdf_configure(ljmd_batch_t *h, int32_t nbins, const double *rmax, int32_t every)
{
    static const char *who = "ljmd_batch_rdf_configure";
    LJMD_TRY(enter(h, who, 0));
    if (nbins < 0 || nbins > kBatchRdfMaxBins)
        return fail(h, LJMD_ERR_INVALID_ARG, "%s: nbins = %d outside 1..%d (0 switches g(r) off)", who, nbins,
                     kBatchRdfMaxBins);
    if (every < 0) return fail(h, LJMD_ERR_INVALID_ARG, "%s: every must be >= 0", who);
    if (nbins > 0 && rmax)
        for (size_t b = 0; b < h->B; ++b)
            if (!(std::isfinite(rmax[b]) && rmax[b] > 0.0))
                return fail(h, LJMD_ERR_INVALID_ARG, "%s: replica %zu: rmax must be finite and > 0", who, b);
    LJMD_HIP(h, hipSetDevice(h->device));
    rdf_release(h);
    if (nbins == 0) return LJMD_OK;
    std::vector<BatchRdfReplica> table;
    LJMD_TRY(host_alloc(h, who, [&] { table.resize(h->B); }));
    for (size_t b = 0; b < h->B; ++b) {
        BatchRdfReplica &e = table[b];
        e.rmax = rmax ? rmax[b] : 0.5 * h->rep[b].L;
        e.dr = e.rmax / nbins;                       // as the reference: dr = rmax / nbins
        e.inv_dr = 1.0 / e.dr;
    }
    const size_t hbytes = h->B * (size_t)nbins * sizeof(unsigned long long), tbytes = h->B * sizeof(BatchRdfReplica);
    auto body = [&]() -> int {
        LJMD_TRY(device_alloc(h, &h->rdf.d_hist, hbytes, who, "histograms"));
        LJMD_TRY(device_alloc(h, &h->rdf.d_table, tbytes, who, "the g(r) table"));
        LJMD_HIP(h, hipMemsetAsync(h->rdf.d_hist, 0, hbytes, h->stream));
        LJMD_HIP(h, hipMemcpyAsync(h->rdf.d_table, table.data(), tbytes, hipMemcpyHostToDevice, h->stream));
        // table goes out of scope: the one configure that waits (ljmd_batch_tcf_configure copies nothing from the host)
        LJMD_HIP(h, hipStreamSynchronize(h->stream));
        return LJMD_OK;
    };
    const int rc_ = body();
    if (rc_ != LJMD_OK) {             // unlike ljmd_batch_tcf_configure, hipGetLastError is not cleared -- kept as it is
        rdf_release(h);
        return rc_;
    }
    h->rdf.nbins = nbins;
    h->rdf.every = every;
    return LJMD_OK;
}

int ljmd_batch_rdf_accumulate(ljmd_batch_t *h)
{
    static const char *who = "ljmd_batch_rdf_accumulate";
    LJMD_TRY(enter(h, who, kNeedRdf | kNeedState | kNeedSound | kNeedDevice));
    return accumulate_now(h, rdf_accumulator(h), who);
}

int ljmd_batch_rdf_read(ljmd_batch_t *h, uint64_t *hist, int64_t *n_snapshots)
{
    static const char *who = "ljmd_batch_rdf_read";
    LJMD_TRY(enter(h, who, kNeedRdf | kNeedDevice));      // a poisoned handle may still be read
    static_assert(sizeof(uint64_t) == sizeof(unsigned long long), "histogram word");
    if (hist)
        LJMD_HIP(h, hipMemcpyAsync(hist, h->rdf.d_hist, h->B * (size_t)h->rdf.nbins * sizeof(uint64_t),
                                    hipMemcpyDeviceToHost, h->stream));
    const hipError_t e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess)
        return poison(h, LJMD_ERR_HIP, "%s: kernel or copy failed: %s; the handle is poisoned until ljmd_batch_set_state",
                      who, hipGetErrorString(e));
    if (n_snapshots) *n_snapshots = h->rdf.snapshots;
    return LJMD_OK;
}

int ljmd_batch_rdf_reset(ljmd_batch_t *h)
{
    static const char *who = "ljmd_batch_rdf_reset";
    LJMD_TRY(enter(h, who, kNeedRdf | kNeedDevice));
    LJMD_HIP(h, hipMemsetAsync(h->rdf.d_hist, 0, h->B * (size_t)h->rdf.nbins * sizeof(unsigned long long), h->stream));
    h->rdf.snapshots = 0;
    return LJMD_OK;
}

}  // extern "C"
