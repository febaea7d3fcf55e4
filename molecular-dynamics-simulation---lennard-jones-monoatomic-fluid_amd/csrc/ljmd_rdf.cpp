// ljmd_rdf.cpp -- host core of the engine's resident g(r) accumulation (kernels: ljmd_rdf.hip): guards, sizes, argument
// blocks, launches, reads and resets.  It sees an engine only through ResidentView and links without anything of struct
// ljmd (tests/rdf_host); the C entry points are in ljmd_resident.cpp.
#include "ljmd_resident.h"

#include <algorithm>
#include <cmath>
#include <vector>

using namespace ljmdh;

namespace ljmdr {

namespace {

// the buffers of a state in the order they are allocated; the sizes matter to configure only
std::array<DeviceBuffer, 3> buffers(RdfState *st, int nbins = 0, int T = 0)
{
    return {{{(void **)&st->d_hist, (size_t)nbins * sizeof(unsigned long long), "the histogram"},
             {(void **)&st->d_count, 2 * sizeof(unsigned long long), "the tile-pair counters"},
             {(void **)&st->d_bbox, (size_t)T * kRdfBoxStride * sizeof(double), "the tile boxes"}}};
}

}  // namespace

int not_configured(std::string *err, const char *who)
{
    return fail(err, LJMD_ERR_STATE, "%s: g(r) is not configured (call ljmd_rdf_configure first)", who);
}

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
    free_buffers(buffers(st), stream);
    st->timer.destroy();
    *st = {};
}

int rdf_configure(RdfState *st, std::string *err, const char *who, const ResidentView &v, int32_t nbins, double rmax)
{
    if (nbins < 0 || nbins > kRdfMaxBins)
        return fail(err, LJMD_ERR_INVALID_ARG, "%s: nbins = %d outside 1..%d (0 switches g(r) off)", who, nbins, kRdfMaxBins);
    if (nbins > 0 && !(std::isfinite(rmax) && rmax > 0.0))
        return fail(err, LJMD_ERR_INVALID_ARG, "%s: rmax must be finite and > 0", who);
    rdf_release(st, v.stream);
    if (nbins == 0) return LJMD_OK;
    const auto bufs = buffers(st, nbins, v.T);
    auto body = [&]() -> int {
        LJMD_TRY(alloc_buffers(err, who, bufs));
        LJMD_HIP(err, st->timer.create());
        LJMD_HIP(err, hipMemsetAsync(st->d_hist, 0, bufs[0].bytes, v.stream));
        LJMD_HIP(err, hipMemsetAsync(st->d_count, 0, bufs[1].bytes, v.stream));
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

int rdf_accumulate(RdfState *st, std::string *err, const char *who, const ResidentView &v)
{
    if (st->nbins == 0) return not_configured(err, who);
    const RdfWalk w = rdf_plan_walk(v.TB, v.T, v.G, v.walk_chunk);
    // a 32-bit LDS bin cannot overflow: rdf_plan_walk caps the slice; checked, not assumed
    if (rdf_lds_bound(w.chunk, w.weight) > 0xffffffffull)
        return fail(err, LJMD_ERR_RANGE, "%s: a slice of %d column tiles could overflow a 32-bit histogram bin", who, w.chunk);
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
    LJMD_HIP(err, hipMemsetAsync(st->d_count, 0, 2 * sizeof(unsigned long long), v.stream));
    LJMD_HIP(err, st->timer.start(v.stream));
    hipError_t e = launch_rdf_boxes(ba, v.stream);
    if (e == hipSuccess) e = launch_rdf_pairs(pa, dim3(w.row_blocks, w.slices), v.stream);
    if (e != hipSuccess) return fail(err, LJMD_ERR_HIP, "%s: g(r) launch failed: %s", who, hipGetErrorString(e));
    LJMD_HIP(err, st->timer.stop(v.stream));
    ++st->snapshots;
    return LJMD_OK;
}

int rdf_read(RdfState *st, std::string *err, const char *who, const ResidentView &v, uint64_t *hist, int64_t *n_snapshots)
{
    if (st->nbins == 0) return not_configured(err, who);
    static_assert(sizeof(uint64_t) == sizeof(unsigned long long), "histogram word");
    if (hist)
        LJMD_HIP(err, hipMemcpyAsync(hist, st->d_hist, (size_t)st->nbins * sizeof(uint64_t), hipMemcpyDeviceToHost, v.stream));
    LJMD_HIP(err, hipStreamSynchronize(v.stream));
    if (n_snapshots) *n_snapshots = st->snapshots;
    return LJMD_OK;
}

int rdf_reset(RdfState *st, std::string *err, const char *who, const ResidentView &v)
{
    if (st->nbins == 0) return not_configured(err, who);
    LJMD_HIP(err, hipMemsetAsync(st->d_hist, 0, (size_t)st->nbins * sizeof(unsigned long long), v.stream));
    st->snapshots = 0;
    return LJMD_OK;
}

int rdf_profile_read(RdfState *st, std::string *err, const char *who, const ResidentView &v, int64_t *visited, int64_t *total,
                     double *kernel_ms)
{
    if (st->nbins == 0) return not_configured(err, who);
    unsigned long long c[2] = {0, 0};
    float ms = 0.0f;
    if (st->timer.timed) LJMD_HIP(err, hipMemcpyAsync(c, st->d_count, sizeof c, hipMemcpyDeviceToHost, v.stream));
    LJMD_HIP(err, st->timer.elapsed_ms(v.stream, &ms));
    if (visited) *visited = (int64_t)c[0];
    if (total) *total = (int64_t)c[1];
    if (kernel_ms) *kernel_ms = (double)ms;
    return LJMD_OK;
}

}  // namespace ljmdr
