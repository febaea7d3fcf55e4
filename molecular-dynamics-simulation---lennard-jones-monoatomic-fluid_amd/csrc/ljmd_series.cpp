// ljmd_series.cpp -- the one host core of the engine's resident series observables, the pressure tensor
// (ljmd_stress.cpp) and the heat flux (ljmd_heatflux.cpp): guards, sizes, buffers, the launches of one accumulate, reads
// and resets, driven by the observable's SeriesDesc (ljmd_resident.h).  The core sees an engine only through
// ResidentView, references no launcher but launch_rdf_boxes, and links without anything of struct ljmd
// (tests/stress_host, tests/heatflux_host).
#include "ljmd_resident.h"

#include <new>

namespace ljmdh {

namespace {

enum { kSeries, kPart, kKpart, kPcount, kCount, kPflag, kKflag, kRange, kBbox, kBuffers };

// the buffers of a state in the order they are allocated; the sizes matter to configure only
std::array<DeviceBuffer, kBuffers> buffers(const SeriesDesc &d, SeriesState *st, int max_snapshots = 0, int workgroups = 0,
                                           int blocks = 0, int T = 0)
{
    const size_t word = 3 * sizeof(uint64_t);
    return {{{(void **)&st->d_series, (size_t)max_snapshots * d.words * sizeof(uint64_t), "the series"},
             {(void **)&st->d_part, (size_t)workgroups * d.pair_components * word, "the pair partials"},
             {(void **)&st->d_kpart, (size_t)blocks * d.particle_components * word, d.particle_partials},
             {(void **)&st->d_pcount, (size_t)workgroups * 2 * sizeof(unsigned long long), "the tile-pair partials"},
             {(void **)&st->d_count, 2 * sizeof(unsigned long long), "the tile-pair counters"},
             {(void **)&st->d_pflag, (size_t)workgroups * sizeof(unsigned), "the pair flags"},
             {(void **)&st->d_kflag, (size_t)blocks * sizeof(unsigned), d.particle_flags},
             {(void **)&st->d_range, sizeof(int32_t), "the range word"},
             {(void **)&st->d_bbox, (size_t)T * ljmdr::kRdfBoxStride * sizeof(double), "the tile boxes"}}};
}

int kinetic_blocks(const SeriesDesc &d, const ResidentView &v) { return (v.P + d.kin_block - 1) / d.kin_block; }

}  // namespace

int series_not_configured(const SeriesDesc &d, std::string *err, const char *who)
{
    return fail(err, LJMD_ERR_STATE, "%s: the %s is not configured (call ljmd_%s_configure first)", who, d.phrase, d.tag);
}

void series_release(const SeriesDesc &d, SeriesState *st, hipStream_t stream)
{
    free_buffers(buffers(d, st), stream);
    st->timer.destroy();
    *st = {};
}

int series_configure(const SeriesDesc &d, SeriesState *st, std::string *err, const char *who, const ResidentView &v,
                     int32_t max_snapshots)
{
    if (max_snapshots < 0 || max_snapshots > d.max_snapshots)
        return fail(err, LJMD_ERR_INVALID_ARG, "%s: max_snapshots = %d outside 1..%d (0 switches the %s off)", who,
                    max_snapshots, d.max_snapshots, d.phrase);
    if (d.one_rank && max_snapshots > 0 && (v.multi || v.G != 1))
        return fail(err, LJMD_ERR_INVALID_ARG, "%s: n_ranks = %d%s: a pair term needs the velocities of both particles and a "
                                               "rank holds only its own, so the %s of the resident system needs a "
                                               "one-rank engine (ljmd_create with n_ranks = 1)", who, v.G,
                    v.multi ? " (multi-device handle)" : "", d.phrase);
    if (max_snapshots > 0 && (v.n < 1 || v.n > d.max_n))
        return fail(err, LJMD_ERR_INVALID_ARG, "%s: n = %d outside 1..%d", who, v.n, d.max_n);
    series_release(d, st, v.stream);
    if (max_snapshots == 0) return LJMD_OK;
    const ljmdr::RdfWalk w = ljmdr::rdf_plan_walk(v.TB, v.T, v.G, v.walk_chunk);
    const int workgroups = w.row_blocks * w.slices;
    const int blocks = kinetic_blocks(d, v);
    const auto bufs = buffers(d, st, max_snapshots, workgroups, blocks, v.T);
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
        series_release(d, st, v.stream);
        return rc_;
    }
    st->max_snapshots = max_snapshots;
    st->workgroups = workgroups;
    st->blocks = blocks;
    return LJMD_OK;
}

int series_accumulate(const SeriesDesc &d, SeriesState *st, std::string *err, const char *who, const ResidentView &v)
{
    if (st->max_snapshots == 0) return series_not_configured(d, err, who);
    if (st->snapshots >= st->max_snapshots)
        return fail(err, LJMD_ERR_STATE, "%s: the series is full (%d snapshots; read it, then ljmd_%s_reset)", who,
                    st->max_snapshots, d.tag);
    const ljmdr::RdfWalk w = ljmdr::rdf_plan_walk(v.TB, v.T, v.G, v.walk_chunk);
    const int blocks = kinetic_blocks(d, v);
    if ((d.one_rank && (v.G != 1 || v.multi)) || w.row_blocks * w.slices != st->workgroups || blocks != st->blocks || !v.pos ||
        !v.v)
        return fail(err, LJMD_ERR_STATE, "%s: the engine is not the one the %s was configured for", who, d.phrase);
    ljmdr::RdfBoxArgs ba{};
    ba.pos = v.pos;
    ba.bbox = st->d_bbox;
    ba.P = v.P; ba.TB = v.TB; ba.T = v.T;
    ljmdk::SeriesKineticArgs ka{};
    ka.v = v.v;
    ka.kpart = st->d_kpart; ka.kflag = st->d_kflag;
    ka.P = v.P; ka.blocks = blocks;
    ljmdk::SeriesFoldArgs fa{};
    fa.part = st->d_part; fa.pcount = st->d_pcount; fa.pflag = st->d_pflag;
    fa.kpart = st->d_kpart; fa.kflag = st->d_kflag;
    fa.workgroups = st->workgroups; fa.blocks = blocks;
    fa.row = st->d_series + (size_t)st->snapshots * d.words;
    fa.count = st->d_count;
    fa.range = st->d_range;
    LJMD_HIP(err, st->timer.start(v.stream));
    hipError_t e = ljmdr::launch_rdf_boxes(ba, v.stream);
    if (e == hipSuccess) e = d.launch(*st, v, w, ka, fa);
    if (e != hipSuccess) return fail(err, LJMD_ERR_HIP, "%s: %s launch failed: %s", who, d.phrase, hipGetErrorString(e));
    LJMD_HIP(err, st->timer.stop(v.stream));
    ++st->snapshots;
    return LJMD_OK;
}

int series_fetch(const SeriesDesc &d, SeriesState *st, std::string *err, const char *who, const ResidentView &v, int64_t *words,
                 int64_t *n_snapshots)
{
    if (st->max_snapshots == 0) return series_not_configured(d, err, who);
    int32_t range = 0;
    LJMD_HIP(err, hipMemcpyAsync(&range, st->d_range, sizeof range, hipMemcpyDeviceToHost, v.stream));
    if (words && st->snapshots > 0)
        LJMD_HIP(err, hipMemcpyAsync(words, st->d_series, (size_t)st->snapshots * d.words * sizeof(uint64_t),
                                       hipMemcpyDeviceToHost, v.stream));
    LJMD_HIP(err, hipStreamSynchronize(v.stream));
    // the handle is not poisoned: the trajectory itself is sound
    if (range != 0)
        return fail(err, LJMD_ERR_RANGE, "%s: a pair's or a particle's %s terms were not finite or |term| >= 2^40 "
                                         "and entered as 0; the flag stays until ljmd_%s_reset", who, d.phrase, d.tag);
    if (n_snapshots) *n_snapshots = st->snapshots;
    return LJMD_OK;
}

int series_read_words(const SeriesDesc &d, SeriesState *st, std::string *err, const char *who, const ResidentView &v, bool want,
                      std::vector<int64_t> *w, int64_t *n_snapshots)
{
    if (st->max_snapshots == 0) return series_not_configured(d, err, who);
    if (want) {
        try {
            w->resize((size_t)st->snapshots * d.words);
        } catch (const std::bad_alloc &) {
            return fail(err, LJMD_ERR_ALLOC, "%s: out of host memory", who);
        }
    }
    return series_fetch(d, st, err, who, v, want ? w->data() : nullptr, n_snapshots);
}

int series_reset(const SeriesDesc &d, SeriesState *st, std::string *err, const char *who, const ResidentView &v)
{
    if (st->max_snapshots == 0) return series_not_configured(d, err, who);
    LJMD_HIP(err, hipMemsetAsync(st->d_series, 0, (size_t)st->max_snapshots * d.words * sizeof(uint64_t), v.stream));
    LJMD_HIP(err, hipMemsetAsync(st->d_range, 0, sizeof(int32_t), v.stream));
    st->snapshots = 0;
    return LJMD_OK;
}

int series_profile_read(const SeriesDesc &d, SeriesState *st, std::string *err, const char *who, const ResidentView &v,
                        int64_t *visited, int64_t *total, double *kernel_ms)
{
    if (st->max_snapshots == 0) return series_not_configured(d, err, who);
    unsigned long long c[2] = {0, 0};
    float ms = 0.0f;
    if (st->timer.timed) LJMD_HIP(err, hipMemcpyAsync(c, st->d_count, sizeof c, hipMemcpyDeviceToHost, v.stream));
    LJMD_HIP(err, st->timer.elapsed_ms(v.stream, &ms));
    if (visited) *visited = (int64_t)c[0];
    if (total) *total = (int64_t)c[1];
    if (kernel_ms) *kernel_ms = (double)ms;
    return LJMD_OK;
}

}  // namespace ljmdh
