// ljmd_rdf.cpp -- host side of the engine's resident g(r) accumulation (include/ljmd.h: ljmd_rdf_*; kernels:
// ljmd_rdf.hip).  Two layers: the core (namespace ljmdr), which sees an engine only through RdfView and links without
// anything of struct ljmd (tests/rdf_host), and the C entry points, which run the entry checks, build the view and
// dispatch a multi-device parent to its rank engines.
#include "ljmd_rdf.h"

#include "ljmd_common.h"

#include <algorithm>
#include <cmath>
#include <vector>

using namespace ljmdh;

namespace ljmdr {

namespace {

int rfail(std::string *err, int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    failv(err, code, fmt, ap);
    va_end(ap);
    return code;
}

#define RDF_HIP(err, call)                                                                                          \
    do {                                                                                                            \
        hipError_t e_ = (call);                                                                                     \
        if (e_ != hipSuccess)                                                                                       \
            return rfail((err), LJMD_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

int not_configured(std::string *err, const char *who)
{
    return rfail(err, LJMD_ERR_STATE, "%s: g(r) is not configured (call ljmd_rdf_configure first)", who);
}

}  // namespace

RdfWalk rdf_plan_walk(int TB, int T, int G, std::optional<int> walk_chunk)
{
    RdfWalk w;
    w.weight = G == 1 ? 2 : 1;
    w.U = G == 1 ? T / 2 + 1 : T;
    w.row_blocks = (TB + kRdfWaves - 1) / kRdfWaves;
    const int want = std::max(1, std::min(w.U, (kRdfTargetWorkgroups + w.row_blocks - 1) / w.row_blocks));
    w.chunk = std::min((w.U + want - 1) / want, kRdfMaxChunk);
    if (walk_chunk) w.chunk = std::max(1, std::min(*walk_chunk, std::min(w.U, kRdfMaxChunk)));
    w.slices = (w.U + w.chunk - 1) / w.chunk;
    return w;
}

void rdf_release(RdfState *st, hipStream_t stream)
{
    if (stream && (st->d_hist || st->d_count || st->d_bbox)) (void)hipStreamSynchronize(stream);
    if (st->d_hist) (void)hipFree(st->d_hist);
    if (st->d_count) (void)hipFree(st->d_count);
    if (st->d_bbox) (void)hipFree(st->d_bbox);
    if (st->ev0) (void)hipEventDestroy(st->ev0);
    if (st->ev1) (void)hipEventDestroy(st->ev1);
    *st = {};
}

int rdf_configure(RdfState *st, std::string *err, const char *who, const RdfView &v, int32_t nbins, double rmax)
{
    if (nbins < 0 || nbins > kRdfMaxBins)
        return rfail(err, LJMD_ERR_INVALID_ARG, "%s: nbins = %d outside 1..%d (0 switches g(r) off)", who, nbins, kRdfMaxBins);
    if (nbins > 0 && !(std::isfinite(rmax) && rmax > 0.0))
        return rfail(err, LJMD_ERR_INVALID_ARG, "%s: rmax must be finite and > 0", who);
    rdf_release(st, v.stream);
    if (nbins == 0) return LJMD_OK;
    const size_t hbytes = (size_t)nbins * sizeof(unsigned long long), cbytes = 2 * sizeof(unsigned long long);
    const size_t bbytes = (size_t)v.T * kRdfBoxStride * sizeof(double);
    auto body = [&]() -> int {
        void **bufs[3] = {(void **)&st->d_hist, (void **)&st->d_count, (void **)&st->d_bbox};
        const size_t sizes[3] = {hbytes, cbytes, bbytes};
        const char *names[3] = {"the histogram", "the tile-pair counters", "the tile boxes"};
        for (int k = 0; k < 3; ++k)
            if (hipMalloc(bufs[k], sizes[k]) != hipSuccess) {
                *bufs[k] = nullptr;
                (void)hipGetLastError();
                return rfail(err, LJMD_ERR_ALLOC, "%s: out of device memory for %s (%zu bytes)", who, names[k], sizes[k]);
            }
        RDF_HIP(err, hipEventCreate(&st->ev0));
        RDF_HIP(err, hipEventCreate(&st->ev1));
        RDF_HIP(err, hipMemsetAsync(st->d_hist, 0, hbytes, v.stream));
        RDF_HIP(err, hipMemsetAsync(st->d_count, 0, cbytes, v.stream));
        return LJMD_OK;
    };
    const int rc_ = body();
    if (rc_ != LJMD_OK) {
        rdf_release(st, v.stream);
        return rc_;
    }
    st->nbins = nbins;
    st->rmax = rmax;
    st->dr = rmax / nbins;                          // as the reference: dr = rmax / nbins
    st->inv_dr = 1.0 / st->dr;
    return LJMD_OK;
}

int rdf_accumulate(RdfState *st, std::string *err, const char *who, const RdfView &v)
{
    if (st->nbins == 0) return not_configured(err, who);
    const RdfWalk w = rdf_plan_walk(v.TB, v.T, v.G, v.walk_chunk);
    // a 32-bit LDS bin cannot overflow: rdf_plan_walk caps the slice; checked, not assumed
    if (rdf_lds_bound(w.chunk, w.weight) > 0xffffffffull)
        return rfail(err, LJMD_ERR_RANGE, "%s: a slice of %d column tiles could overflow a 32-bit histogram bin", who, w.chunk);
    RdfBoxArgs ba{};
    ba.pos = v.pos;
    ba.bbox = st->d_bbox;
    ba.P = v.P; ba.TB = v.TB; ba.T = v.T;
    RdfPairArgs pa{};
    pa.pos = v.pos;
    pa.bbox = st->d_bbox;
    pa.hist = st->d_hist;
    pa.count = st->d_count;
    pa.P = v.P; pa.G = v.G; pa.rank = v.rank; pa.TB = v.TB; pa.T = v.T;
    pa.U = w.U; pa.chunk = w.chunk;
    pa.nbins = st->nbins;
    pa.skip = v.compact ? 1 : 0;
    pa.L = v.L; pa.invL = v.invL;
    pa.rmax = st->rmax; pa.dr = st->dr; pa.inv_dr = st->inv_dr;
    pa.rmax2_skin = st->rmax * st->rmax * (1.0 + 1e-10);
    pa.rmax2_up = st->rmax * st->rmax * (1.0 + 0x1p-50);     // the product is within 2^-53 of rmax^2: this lies above it
    RDF_HIP(err, hipMemsetAsync(st->d_count, 0, 2 * sizeof(unsigned long long), v.stream));
    RDF_HIP(err, hipEventRecord(st->ev0, v.stream));
    hipError_t e = launch_rdf_boxes(ba, v.stream);
    if (e == hipSuccess) e = launch_rdf_pairs(pa, dim3(w.row_blocks, w.slices), v.stream);
    if (e != hipSuccess) return rfail(err, LJMD_ERR_HIP, "%s: g(r) launch failed: %s", who, hipGetErrorString(e));
    RDF_HIP(err, hipEventRecord(st->ev1, v.stream));
    st->timed = true;
    ++st->snapshots;
    return LJMD_OK;
}

int rdf_read(RdfState *st, std::string *err, const char *who, const RdfView &v, uint64_t *hist, int64_t *n_snapshots)
{
    if (st->nbins == 0) return not_configured(err, who);
    static_assert(sizeof(uint64_t) == sizeof(unsigned long long), "histogram word");
    if (hist)
        RDF_HIP(err, hipMemcpyAsync(hist, st->d_hist, (size_t)st->nbins * sizeof(uint64_t), hipMemcpyDeviceToHost, v.stream));
    RDF_HIP(err, hipStreamSynchronize(v.stream));
    if (n_snapshots) *n_snapshots = st->snapshots;
    return LJMD_OK;
}

int rdf_reset(RdfState *st, std::string *err, const char *who, const RdfView &v)
{
    if (st->nbins == 0) return not_configured(err, who);
    RDF_HIP(err, hipMemsetAsync(st->d_hist, 0, (size_t)st->nbins * sizeof(unsigned long long), v.stream));
    st->snapshots = 0;
    return LJMD_OK;
}

int rdf_profile_read(RdfState *st, std::string *err, const char *who, const RdfView &v, int64_t *visited, int64_t *total,
                     double *kernel_ms)
{
    if (st->nbins == 0) return not_configured(err, who);
    unsigned long long c[2] = {0, 0};
    float ms = 0.0f;
    if (st->timed) {
        RDF_HIP(err, hipMemcpyAsync(c, st->d_count, sizeof c, hipMemcpyDeviceToHost, v.stream));
        RDF_HIP(err, hipStreamSynchronize(v.stream));
        RDF_HIP(err, hipEventElapsedTime(&ms, st->ev0, st->ev1));
    }
    if (visited) *visited = (int64_t)c[0];
    if (total) *total = (int64_t)c[1];
    if (kernel_ms) *kernel_ms = (double)ms;
    return LJMD_OK;
}

}  // namespace ljmdr

// ---- C ABI: compiled with the engine; the host test links the core alone (tests/rdf_host: -DLJMD_RDF_CORE_ONLY) ----
#ifndef LJMD_RDF_CORE_ONLY

#include "ljmd_engine.h"
#include "ljmd_multi.h"

namespace {

using ljmdr::RdfView;

RdfView view_of(const ljmd_t *h)
{
    RdfView v;
    v.n = h->n; v.S = h->plan.S; v.P = h->plan.P; v.TB = h->plan.TB; v.T = h->plan.T; v.G = h->G; v.rank = h->rank;
    v.L = h->L; v.invL = h->invL;
    v.pos = h->d_pos;
    v.stream = h->stream;
    v.compact = h->positions_compact;
    v.walk_chunk = h->knobs.walk_chunk;
    return v;
}

// f(rank engine) on every rank of a multi-device parent, the rank's device current; a child's error becomes the parent's
template <class F>
int for_ranks(ljmd_t *h, F &&f)
{
    for (int g = 0; g < h->G; ++g) {
        ljmd_t *e = ljmdm::rank_engine(h, g);
        if (!e) return fail(h, LJMD_ERR_STATE, "multi-device handle without rank %d", g);
        LJMD_HIP(h, hipSetDevice(e->device));
        const int rc_ = f(e);
        if (rc_ != LJMD_OK) return fail(h, rc_, "rank %d (device %d): %s", e->rank, e->device, e->err.c_str());
    }
    return LJMD_OK;
}

}  // namespace

extern "C" {

int ljmd_rdf_configure(ljmd_t *h, int32_t nbins, double rmax)
{
    static const char *who = "ljmd_rdf_configure";
    static_assert(LJMD_RDF_MAX_BINS == ljmdr::kRdfMaxBins, "LJMD_RDF_MAX_BINS out of sync with the kernel");
    LJMD_TRY(entry_checks(h, who, kHandle));
    if (h->multi) {
        // every rank runs the same guards on the same arguments: a failed guard stops at rank 0 with nothing changed
        const int rc_ = for_ranks(h, [&](ljmd_t *e) { return ljmd_rdf_configure(e, nbins, rmax); });
        if (rc_ == LJMD_ERR_INVALID_ARG) return rc_;
        if (rc_ != LJMD_OK) {                       // off everywhere; the first failure's message stays
            const std::string msg = h->err;
            (void)for_ranks(h, [](ljmd_t *e) { return ljmd_rdf_configure(e, 0, 0.0); });
            h->err = msg;
        }
        h->rdf.nbins = rc_ == LJMD_OK ? nbins : 0;
        return rc_;
    }
    LJMD_HIP(h, hipSetDevice(h->device));
    return ljmdr::rdf_configure(&h->rdf, &h->err, who, view_of(h), nbins, rmax);
}

int ljmd_rdf_accumulate(ljmd_t *h)
{
    static const char *who = "ljmd_rdf_accumulate";
    LJMD_TRY(entry_checks(h, who, kHandle));
    if (h->rdf.nbins == 0) return fail(h, LJMD_ERR_STATE, "%s: g(r) is not configured (call ljmd_rdf_configure first)", who);
    LJMD_TRY(entry_checks(h, who, kHaveState | kHaveAccel | kNotPoisoned));
    if (h->multi) return for_ranks(h, [](ljmd_t *e) { return ljmd_rdf_accumulate(e); });
    // between ljmd_step_begin and ljmd_step_finish the own block is a step ahead of the other ranks' blocks
    if (h->step_open || h->forces_pending)
        return fail(h, LJMD_ERR_STATE, "%s: inside a split-phase step (call ljmd_step_finish first)", who);
    LJMD_HIP(h, hipSetDevice(h->device));
    return ljmdr::rdf_accumulate(&h->rdf, &h->err, who, view_of(h));
}

int ljmd_rdf_read(ljmd_t *h, uint64_t *hist, int64_t *n_snapshots)
{
    static const char *who = "ljmd_rdf_read";
    LJMD_TRY(entry_checks(h, who, kHandle));
    if (!h->multi) {
        LJMD_HIP(h, hipSetDevice(h->device));
        return ljmdr::rdf_read(&h->rdf, &h->err, who, view_of(h), hist, n_snapshots);
    }
    if (h->rdf.nbins == 0) return fail(h, LJMD_ERR_STATE, "%s: g(r) is not configured (call ljmd_rdf_configure first)", who);
    // the sum of the ranks' partial histograms; the snapshot count is common to them
    const size_t nbins = (size_t)h->rdf.nbins;
    std::vector<uint64_t> part;
    try {
        part.resize(nbins);
    } catch (const std::bad_alloc &) {
        return fail(h, LJMD_ERR_ALLOC, "%s: out of host memory", who);
    }
    if (hist) std::fill(hist, hist + nbins, (uint64_t)0);
    return for_ranks(h, [&](ljmd_t *e) {
        const int rc_ = ljmd_rdf_read(e, hist ? part.data() : nullptr, n_snapshots);
        if (rc_ == LJMD_OK && hist)
            for (size_t b = 0; b < nbins; ++b) hist[b] += part[b];
        return rc_;
    });
}

int ljmd_rdf_reset(ljmd_t *h)
{
    static const char *who = "ljmd_rdf_reset";
    LJMD_TRY(entry_checks(h, who, kHandle));
    if (h->multi) {
        if (h->rdf.nbins == 0) return fail(h, LJMD_ERR_STATE, "%s: g(r) is not configured (call ljmd_rdf_configure first)", who);
        return for_ranks(h, [](ljmd_t *e) { return ljmd_rdf_reset(e); });
    }
    LJMD_HIP(h, hipSetDevice(h->device));
    return ljmdr::rdf_reset(&h->rdf, &h->err, who, view_of(h));
}

int ljmd_rdf_profile_read(ljmd_t *h, int64_t *tile_pairs_visited, int64_t *tile_pairs_total, double *kernel_ms)
{
    static const char *who = "ljmd_rdf_profile_read";
    LJMD_TRY(entry_checks(h, who, kHandle));
    if (!h->multi) {
        LJMD_HIP(h, hipSetDevice(h->device));
        return ljmdr::rdf_profile_read(&h->rdf, &h->err, who, view_of(h), tile_pairs_visited, tile_pairs_total, kernel_ms);
    }
    if (h->rdf.nbins == 0) return fail(h, LJMD_ERR_STATE, "%s: g(r) is not configured (call ljmd_rdf_configure first)", who);
    // tile pairs: sums over the ranks; time: the slowest rank
    int64_t vis = 0, tot = 0;
    double ms = 0.0;
    const int rc_ = for_ranks(h, [&](ljmd_t *e) {
        int64_t a = 0, b = 0;
        double t = 0.0;
        const int r = ljmd_rdf_profile_read(e, &a, &b, &t);
        vis += a; tot += b; ms = std::max(ms, t);
        return r;
    });
    if (rc_ != LJMD_OK) return rc_;
    if (tile_pairs_visited) *tile_pairs_visited = vis;
    if (tile_pairs_total) *tile_pairs_total = tot;
    if (kernel_ms) *kernel_ms = ms;
    return LJMD_OK;
}

}  // extern "C"

#endif  // LJMD_RDF_CORE_ONLY
