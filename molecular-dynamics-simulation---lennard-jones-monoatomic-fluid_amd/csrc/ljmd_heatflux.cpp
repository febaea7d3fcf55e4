// ljmd_heatflux.cpp -- host core of the engine's resident heat flux (kernels: ljmd_heatflux.hip): guards, sizes, argument
// blocks, launches, reads and resets, and ljmd_heatflux_from_exact, which needs no engine.  The core sees an engine only
// through ResidentView and links without anything of struct ljmd (tests/heatflux_host); the C entry points that take a
// handle are in ljmd_resident.cpp.
#include "ljmd_resident.h"

#include <algorithm>
#include <cmath>
#include <new>
#include <vector>

using namespace ljmdh;

namespace ljmdq {

namespace {

enum { kSeries, kPart, kKpart, kPcount, kCount, kPflag, kKflag, kRange, kBbox, kBuffers };

// the buffers of a state in the order they are allocated; the sizes matter to configure only
std::array<DeviceBuffer, kBuffers> buffers(HeatfluxState *st, int max_snapshots = 0, int workgroups = 0, int blocks = 0, int T = 0)
{
    const size_t word = 3 * sizeof(uint64_t);
    return {{{(void **)&st->d_series, (size_t)max_snapshots * kHeatfluxWords * sizeof(uint64_t), "the series"},
             {(void **)&st->d_part, (size_t)workgroups * kHeatfluxPairComponents * word, "the pair partials"},
             {(void **)&st->d_kpart, (size_t)blocks * kHeatfluxKinComponents * word, "the convective partials"},
             {(void **)&st->d_pcount, (size_t)workgroups * 2 * sizeof(unsigned long long), "the tile-pair partials"},
             {(void **)&st->d_count, 2 * sizeof(unsigned long long), "the tile-pair counters"},
             {(void **)&st->d_pflag, (size_t)workgroups * sizeof(unsigned), "the pair flags"},
             {(void **)&st->d_kflag, (size_t)blocks * sizeof(unsigned), "the convective flags"},
             {(void **)&st->d_range, sizeof(int32_t), "the range word"},
             {(void **)&st->d_bbox, (size_t)T * kRdfBoxStride * sizeof(double), "the tile boxes"}}};
}

}  // namespace

int not_configured(std::string *err, const char *who)
{
    return fail(err, LJMD_ERR_STATE, "%s: the heat flux is not configured (call ljmd_heatflux_configure first)", who);
}

void heatflux_release(HeatfluxState *st, hipStream_t stream)
{
    free_buffers(buffers(st), stream);
    st->timer.destroy();
    *st = {};
}

int heatflux_configure(HeatfluxState *st, std::string *err, const char *who, const ResidentView &v, int32_t max_snapshots)
{
    static_assert(kHeatfluxMaxSnapshots == LJMD_HEATFLUX_MAX_SNAPSHOTS, "LJMD_HEATFLUX_MAX_SNAPSHOTS out of sync with the core");
    static_assert(kHeatfluxMaxN == ljmdk::kFixedMaxN, "the lane accumulators rest on kFixedMaxN");
    if (max_snapshots < 0 || max_snapshots > kHeatfluxMaxSnapshots)
        return fail(err, LJMD_ERR_INVALID_ARG, "%s: max_snapshots = %d outside 1..%d (0 switches the heat flux off)", who,
                    max_snapshots, kHeatfluxMaxSnapshots);
    if (max_snapshots > 0 && (v.multi || v.G != 1))
        return fail(err, LJMD_ERR_INVALID_ARG, "%s: n_ranks = %d%s: a pair term needs the velocities of both particles and a "
                                               "rank holds only its own, so the heat flux of the resident system needs a "
                                               "one-rank engine (ljmd_create with n_ranks = 1)", who, v.G,
                    v.multi ? " (multi-device handle)" : "");
    if (max_snapshots > 0 && (v.n < 1 || v.n > kHeatfluxMaxN))
        return fail(err, LJMD_ERR_INVALID_ARG, "%s: n = %d outside 1..%d", who, v.n, kHeatfluxMaxN);
    heatflux_release(st, v.stream);
    if (max_snapshots == 0) return LJMD_OK;
    const ljmdr::RdfWalk w = ljmdr::rdf_plan_walk(v.TB, v.T, v.G, v.walk_chunk);
    const int workgroups = w.row_blocks * w.slices;
    const int blocks = (v.P + kHeatfluxKinBlock - 1) / kHeatfluxKinBlock;
    const auto bufs = buffers(st, max_snapshots, workgroups, blocks, v.T);
    auto body = [&]() -> int {
        LJMD_TRY(alloc_buffers(err, who, bufs));
        LJMD_HIP(err, st->timer.create());
        // the partials and flags are written before they are read; the rest starts at zero
        LJMD_HIP(err, hipMemsetAsync(st->d_series, 0, bufs[kSeries].bytes, v.stream));
        LJMD_HIP(err, hipMemsetAsync(st->d_count, 0, bufs[kCount].bytes, v.stream));
        LJMD_HIP(err, hipMemsetAsync(st->d_range, 0, bufs[kRange].bytes, v.stream));
        return LJMD_OK;
    };
    const int rc_ = body();
    if (rc_ != LJMD_OK) {
        heatflux_release(st, v.stream);
        return rc_;
    }
    st->max_snapshots = max_snapshots;
    st->workgroups = workgroups;
    st->blocks = blocks;
    return LJMD_OK;
}

int heatflux_accumulate(HeatfluxState *st, std::string *err, const char *who, const ResidentView &v)
{
    if (st->max_snapshots == 0) return not_configured(err, who);
    if (st->snapshots >= st->max_snapshots)
        return fail(err, LJMD_ERR_STATE, "%s: the series is full (%d snapshots; read it, then ljmd_heatflux_reset)", who,
                    st->max_snapshots);
    const ljmdr::RdfWalk w = ljmdr::rdf_plan_walk(v.TB, v.T, v.G, v.walk_chunk);
    const int blocks = (v.P + kHeatfluxKinBlock - 1) / kHeatfluxKinBlock;
    if (v.G != 1 || v.multi || w.row_blocks * w.slices != st->workgroups || blocks != st->blocks || !v.pos || !v.v)
        return fail(err, LJMD_ERR_STATE, "%s: the engine is not the one the heat flux was configured for", who);
    ljmdr::RdfBoxArgs ba{};
    ba.pos = v.pos;
    ba.bbox = st->d_bbox;
    ba.P = v.P; ba.TB = v.TB; ba.T = v.T;
    HeatfluxPairArgs pa{};
    pa.pos = v.pos;
    pa.vel = v.v;
    pa.bbox = st->d_bbox;
    pa.part = st->d_part; pa.pcount = st->d_pcount; pa.pflag = st->d_pflag;
    pa.P = v.P; pa.T = v.T;
    pa.U = w.U; pa.chunk = w.chunk;
    pa.skip = v.compact ? 1 : 0;
    pa.L = v.L; pa.invL = v.invL; pa.rc2 = v.rc2;
    pa.rc2_skin = v.rc2 * (1.0 + 1e-10);
    HeatfluxKineticArgs ka{};
    ka.v = v.v;
    ka.kpart = st->d_kpart; ka.kflag = st->d_kflag;
    ka.P = v.P; ka.blocks = blocks;
    HeatfluxFoldArgs fa{};
    fa.part = st->d_part; fa.pcount = st->d_pcount; fa.pflag = st->d_pflag;
    fa.kpart = st->d_kpart; fa.kflag = st->d_kflag;
    fa.workgroups = st->workgroups; fa.blocks = blocks;
    fa.row = st->d_series + (size_t)st->snapshots * kHeatfluxWords;
    fa.count = st->d_count;
    fa.range = st->d_range;
    LJMD_HIP(err, st->timer.start(v.stream));
    hipError_t e = ljmdr::launch_rdf_boxes(ba, v.stream);
    if (e == hipSuccess) e = launch_heatflux_pairs(pa, dim3(w.row_blocks, w.slices), v.stream);
    if (e == hipSuccess) e = launch_heatflux_kinetic(ka, v.stream);
    if (e == hipSuccess) e = launch_heatflux_fold(fa, v.stream);
    if (e != hipSuccess) return fail(err, LJMD_ERR_HIP, "%s: heat flux launch failed: %s", who, hipGetErrorString(e));
    LJMD_HIP(err, st->timer.stop(v.stream));
    ++st->snapshots;
    return LJMD_OK;
}

int heatflux_fetch(HeatfluxState *st, std::string *err, const char *who, const ResidentView &v, int64_t *words, int64_t *n_snapshots)
{
    if (st->max_snapshots == 0) return not_configured(err, who);
    int32_t range = 0;
    LJMD_HIP(err, hipMemcpyAsync(&range, st->d_range, sizeof range, hipMemcpyDeviceToHost, v.stream));
    if (words && st->snapshots > 0)
        LJMD_HIP(err, hipMemcpyAsync(words, st->d_series, (size_t)st->snapshots * kHeatfluxWords * sizeof(uint64_t),
                                       hipMemcpyDeviceToHost, v.stream));
    LJMD_HIP(err, hipStreamSynchronize(v.stream));
    // the handle is not poisoned: the trajectory itself is sound
    if (range != 0)
        return fail(err, LJMD_ERR_RANGE, "%s: a pair's or a particle's heat flux terms were not finite or |term| >= 2^40 "
                                         "and entered as 0; the flag stays until ljmd_heatflux_reset", who);
    if (n_snapshots) *n_snapshots = st->snapshots;
    return LJMD_OK;
}

int heatflux_read(HeatfluxState *st, std::string *err, const char *who, const ResidentView &v, double *j, double *parts,
                  int64_t *n_snapshots)
{
    if (st->max_snapshots == 0) return not_configured(err, who);
    std::vector<int64_t> w;
    const bool want = j || parts;
    if (want) {
        try {
            w.resize((size_t)st->snapshots * kHeatfluxWords);
        } catch (const std::bad_alloc &) {
            return fail(err, LJMD_ERR_ALLOC, "%s: out of host memory", who);
        }
    }
    LJMD_TRY(heatflux_fetch(st, err, who, v, want ? w.data() : nullptr, n_snapshots));
    for (int64_t s = 0; want && s < st->snapshots; ++s)
        heatflux_doubles(w.data() + (size_t)s * kHeatfluxWords, v.L, j ? j + (size_t)s * 3 : nullptr,
                         parts ? parts + (size_t)s * 9 : nullptr);
    return LJMD_OK;
}

int heatflux_reset(HeatfluxState *st, std::string *err, const char *who, const ResidentView &v)
{
    if (st->max_snapshots == 0) return not_configured(err, who);
    LJMD_HIP(err, hipMemsetAsync(st->d_series, 0, (size_t)st->max_snapshots * kHeatfluxWords * sizeof(uint64_t), v.stream));
    LJMD_HIP(err, hipMemsetAsync(st->d_range, 0, sizeof(int32_t), v.stream));
    st->snapshots = 0;
    return LJMD_OK;
}

int heatflux_profile_read(HeatfluxState *st, std::string *err, const char *who, const ResidentView &v, int64_t *visited,
                          int64_t *total, double *kernel_ms)
{
    if (st->max_snapshots == 0) return not_configured(err, who);
    unsigned long long c[2] = {0, 0};
    float ms = 0.0f;
    if (st->timer.timed) LJMD_HIP(err, hipMemcpyAsync(c, st->d_count, sizeof c, hipMemcpyDeviceToHost, v.stream));
    LJMD_HIP(err, st->timer.elapsed_ms(v.stream, &ms));
    if (visited) *visited = (int64_t)c[0];
    if (total) *total = (int64_t)c[1];
    if (kernel_ms) *kernel_ms = (double)ms;
    return LJMD_OK;
}

}  // namespace ljmdq

extern "C" int ljmd_heatflux_from_exact(const int64_t *words, double box_length, double *j3, double *parts9)
{
    if (!words || !j3) return fail(nullptr, LJMD_ERR_INVALID_ARG, "ljmd_heatflux_from_exact: NULL argument");
    if (!(std::isfinite(box_length) && box_length > 0.0))
        return fail(nullptr, LJMD_ERR_INVALID_ARG, "ljmd_heatflux_from_exact: box_length must be finite and > 0");
    ljmdq::heatflux_doubles(words, box_length, j3, parts9);
    return LJMD_OK;
}
