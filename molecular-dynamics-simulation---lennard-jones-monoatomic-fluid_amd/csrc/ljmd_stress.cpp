// ljmd_stress.cpp -- host side of the engine's resident pressure tensor (include/ljmd.h: ljmd_stress_*; kernels:
// ljmd_stress.hip).  Two layers, as in ljmd_rdf.cpp: the core (namespace ljmds), which sees an engine only through
// StressView and links without anything of struct ljmd (tests/stress_host), and the C entry points, which run the entry
// checks, build the view and dispatch a multi-device parent to its rank engines.
#include "ljmd_stress.h"

#include "ljmd_common.h"
#include "ljmd_internal.h"

#include <algorithm>
#include <cmath>
#include <new>
#include <vector>

using namespace ljmdh;

namespace ljmds {

namespace {

int sfail(std::string *err, int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    failv(err, code, fmt, ap);
    va_end(ap);
    return code;
}

#define STRESS_HIP(err, call)                                                                                       \
    do {                                                                                                            \
        hipError_t e_ = (call);                                                                                     \
        if (e_ != hipSuccess)                                                                                       \
            return sfail((err), LJMD_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

int not_configured(std::string *err, const char *who)
{
    return sfail(err, LJMD_ERR_STATE, "%s: the pressure tensor is not configured (call ljmd_stress_configure first)", who);
}

void **buffers(StressState *st, int k)
{
    void **b[] = {(void **)&st->d_series, (void **)&st->d_part, (void **)&st->d_kpart, (void **)&st->d_pcount,
                  (void **)&st->d_count, (void **)&st->d_pflag, (void **)&st->d_kflag, (void **)&st->d_range,
                  (void **)&st->d_bbox};
    return b[k];
}
constexpr int kBuffers = 9;

}  // namespace

void stress_release(StressState *st, hipStream_t stream)
{
    bool any = false;
    for (int k = 0; k < kBuffers; ++k) any = any || *buffers(st, k);
    if (stream && any) (void)hipStreamSynchronize(stream);
    for (int k = 0; k < kBuffers; ++k)
        if (*buffers(st, k)) (void)hipFree(*buffers(st, k));
    if (st->ev0) (void)hipEventDestroy(st->ev0);
    if (st->ev1) (void)hipEventDestroy(st->ev1);
    *st = {};
}

int stress_configure(StressState *st, std::string *err, const char *who, const StressView &v, int32_t max_snapshots)
{
    static_assert(kStressMaxSnapshots == LJMD_STRESS_MAX_SNAPSHOTS, "LJMD_STRESS_MAX_SNAPSHOTS out of sync with the core");
    static_assert(kStressMaxN == ljmdk::kFixedMaxN, "the lane accumulators rest on kFixedMaxN");
    if (max_snapshots < 0 || max_snapshots > kStressMaxSnapshots)
        return sfail(err, LJMD_ERR_INVALID_ARG, "%s: max_snapshots = %d outside 1..%d (0 switches the pressure tensor off)", who,
                     max_snapshots, kStressMaxSnapshots);
    if (max_snapshots > 0 && (v.n < 1 || v.n > kStressMaxN))
        return sfail(err, LJMD_ERR_INVALID_ARG, "%s: n = %d outside 1..%d", who, v.n, kStressMaxN);
    stress_release(st, v.stream);
    if (max_snapshots == 0) return LJMD_OK;
    const ljmdr::RdfWalk w = ljmdr::rdf_plan_walk(v.TB, v.T, v.G, v.walk_chunk);
    const int workgroups = w.row_blocks * w.slices;
    const int blocks = (v.P + kStressKinBlock - 1) / kStressKinBlock;
    const size_t row = (size_t)kStressComponents * 3 * sizeof(uint64_t);
    const size_t sizes[kBuffers] = {(size_t)max_snapshots * kStressWords * sizeof(uint64_t),
                                    (size_t)workgroups * row,
                                    (size_t)blocks * row,
                                    (size_t)workgroups * 2 * sizeof(unsigned long long),
                                    2 * sizeof(unsigned long long),
                                    (size_t)workgroups * sizeof(unsigned),
                                    (size_t)blocks * sizeof(unsigned),
                                    sizeof(int32_t),
                                    (size_t)v.T * kRdfBoxStride * sizeof(double)};
    const char *names[kBuffers] = {"the series", "the pair partials", "the kinetic partials", "the tile-pair partials",
                                   "the tile-pair counters", "the pair flags", "the kinetic flags", "the range word",
                                   "the tile boxes"};
    auto body = [&]() -> int {
        for (int k = 0; k < kBuffers; ++k)
            if (hipMalloc(buffers(st, k), sizes[k]) != hipSuccess) {
                *buffers(st, k) = nullptr;
                (void)hipGetLastError();
                return sfail(err, LJMD_ERR_ALLOC, "%s: out of device memory for %s (%zu bytes)", who, names[k], sizes[k]);
            }
        STRESS_HIP(err, hipEventCreate(&st->ev0));
        STRESS_HIP(err, hipEventCreate(&st->ev1));
        // the partials and flags are written before they are read; the rest starts at zero
        STRESS_HIP(err, hipMemsetAsync(st->d_series, 0, sizes[0], v.stream));
        STRESS_HIP(err, hipMemsetAsync(st->d_count, 0, sizes[4], v.stream));
        STRESS_HIP(err, hipMemsetAsync(st->d_range, 0, sizes[7], v.stream));
        return LJMD_OK;
    };
    const int rc_ = body();
    if (rc_ != LJMD_OK) {
        stress_release(st, v.stream);
        return rc_;
    }
    st->max_snapshots = max_snapshots;
    st->workgroups = workgroups;
    st->blocks = blocks;
    return LJMD_OK;
}

int stress_accumulate(StressState *st, std::string *err, const char *who, const StressView &v)
{
    if (st->max_snapshots == 0) return not_configured(err, who);
    if (st->snapshots >= st->max_snapshots)
        return sfail(err, LJMD_ERR_STATE, "%s: the series is full (%d snapshots; read it, then ljmd_stress_reset)", who,
                     st->max_snapshots);
    const ljmdr::RdfWalk w = ljmdr::rdf_plan_walk(v.TB, v.T, v.G, v.walk_chunk);
    const int blocks = (v.P + kStressKinBlock - 1) / kStressKinBlock;
    if (w.row_blocks * w.slices != st->workgroups || blocks != st->blocks || !v.pos || !v.v)
        return sfail(err, LJMD_ERR_STATE, "%s: the engine is not the one the pressure tensor was configured for", who);
    ljmdr::RdfBoxArgs ba{};
    ba.pos = v.pos;
    ba.bbox = st->d_bbox;
    ba.P = v.P; ba.TB = v.TB; ba.T = v.T;
    StressPairArgs pa{};
    pa.pos = v.pos;
    pa.bbox = st->d_bbox;
    pa.part = st->d_part; pa.pcount = st->d_pcount; pa.pflag = st->d_pflag;
    pa.P = v.P; pa.G = v.G; pa.rank = v.rank; pa.TB = v.TB; pa.T = v.T;
    pa.U = w.U; pa.chunk = w.chunk;
    pa.skip = v.compact ? 1 : 0;
    pa.L = v.L; pa.invL = v.invL; pa.rc2 = v.rc2;
    pa.rc2_skin = v.rc2 * (1.0 + 1e-10);
    StressKineticArgs ka{};
    ka.v = v.v;
    ka.kpart = st->d_kpart; ka.kflag = st->d_kflag;
    ka.P = v.P; ka.blocks = blocks;
    StressFoldArgs fa{};
    fa.part = st->d_part; fa.pcount = st->d_pcount; fa.pflag = st->d_pflag;
    fa.kpart = st->d_kpart; fa.kflag = st->d_kflag;
    fa.workgroups = st->workgroups; fa.blocks = blocks;
    fa.row = st->d_series + (size_t)st->snapshots * kStressWords;
    fa.count = st->d_count;
    fa.range = st->d_range;
    STRESS_HIP(err, hipEventRecord(st->ev0, v.stream));
    hipError_t e = ljmdr::launch_rdf_boxes(ba, v.stream);
    if (e == hipSuccess) e = launch_stress_pairs(pa, dim3(w.row_blocks, w.slices), v.stream);
    if (e == hipSuccess) e = launch_stress_kinetic(ka, v.stream);
    if (e == hipSuccess) e = launch_stress_fold(fa, v.stream);
    if (e != hipSuccess) return sfail(err, LJMD_ERR_HIP, "%s: pressure tensor launch failed: %s", who, hipGetErrorString(e));
    STRESS_HIP(err, hipEventRecord(st->ev1, v.stream));
    st->timed = true;
    ++st->snapshots;
    return LJMD_OK;
}

int stress_fetch(StressState *st, std::string *err, const char *who, const StressView &v, int64_t *words, int64_t *n_snapshots)
{
    if (st->max_snapshots == 0) return not_configured(err, who);
    int32_t range = 0;
    STRESS_HIP(err, hipMemcpyAsync(&range, st->d_range, sizeof range, hipMemcpyDeviceToHost, v.stream));
    if (words && st->snapshots > 0)
        STRESS_HIP(err, hipMemcpyAsync(words, st->d_series, (size_t)st->snapshots * kStressWords * sizeof(uint64_t),
                                       hipMemcpyDeviceToHost, v.stream));
    STRESS_HIP(err, hipStreamSynchronize(v.stream));
    // the handle is not poisoned: the trajectory itself is sound
    if (range != 0)
        return sfail(err, LJMD_ERR_RANGE, "%s: a pair's or a particle's pressure tensor terms were not finite or |term| >= 2^40 "
                                          "and entered as 0; the flag stays until ljmd_stress_reset", who);
    if (n_snapshots) *n_snapshots = st->snapshots;
    return LJMD_OK;
}

int stress_read(StressState *st, std::string *err, const char *who, const StressView &v, double *p, int64_t *n_snapshots)
{
    if (st->max_snapshots == 0) return not_configured(err, who);
    std::vector<int64_t> w;
    if (p) {
        try {
            w.resize((size_t)st->snapshots * kStressWords);
        } catch (const std::bad_alloc &) {
            return sfail(err, LJMD_ERR_ALLOC, "%s: out of host memory", who);
        }
    }
    LJMD_TRY(stress_fetch(st, err, who, v, p ? w.data() : nullptr, n_snapshots));
    for (int64_t s = 0; p && s < st->snapshots; ++s)
        stress_doubles(w.data() + (size_t)s * kStressWords, v.L, p + (size_t)s * kStressComponents);
    return LJMD_OK;
}

int stress_reset(StressState *st, std::string *err, const char *who, const StressView &v)
{
    if (st->max_snapshots == 0) return not_configured(err, who);
    STRESS_HIP(err, hipMemsetAsync(st->d_series, 0, (size_t)st->max_snapshots * kStressWords * sizeof(uint64_t), v.stream));
    STRESS_HIP(err, hipMemsetAsync(st->d_range, 0, sizeof(int32_t), v.stream));
    st->snapshots = 0;
    return LJMD_OK;
}

int stress_profile_read(StressState *st, std::string *err, const char *who, const StressView &v, int64_t *visited,
                        int64_t *total, double *kernel_ms)
{
    if (st->max_snapshots == 0) return not_configured(err, who);
    unsigned long long c[2] = {0, 0};
    float ms = 0.0f;
    if (st->timed) {
        STRESS_HIP(err, hipMemcpyAsync(c, st->d_count, sizeof c, hipMemcpyDeviceToHost, v.stream));
        STRESS_HIP(err, hipStreamSynchronize(v.stream));
        STRESS_HIP(err, hipEventElapsedTime(&ms, st->ev0, st->ev1));
    }
    if (visited) *visited = (int64_t)c[0];
    if (total) *total = (int64_t)c[1];
    if (kernel_ms) *kernel_ms = (double)ms;
    return LJMD_OK;
}

}  // namespace ljmds

extern "C" int ljmd_stress_from_exact(const int64_t *words, double box_length, double *out6)
{
    if (!words || !out6) return fail(nullptr, LJMD_ERR_INVALID_ARG, "ljmd_stress_from_exact: NULL argument");
    if (!(std::isfinite(box_length) && box_length > 0.0))
        return fail(nullptr, LJMD_ERR_INVALID_ARG, "ljmd_stress_from_exact: box_length must be finite and > 0");
    ljmds::stress_doubles(words, box_length, out6);
    return LJMD_OK;
}

// ---- C ABI: compiled with the engine; the host test links the core alone (tests/stress_host: -DLJMD_STRESS_CORE_ONLY) ----
#ifndef LJMD_STRESS_CORE_ONLY

#include "ljmd_engine.h"
#include "ljmd_multi.h"

namespace {

using ljmds::kStressWords;
using ljmds::StressView;

StressView view_of(const ljmd_t *h)
{
    StressView v;
    v.n = h->n; v.P = h->plan.P; v.TB = h->plan.TB; v.T = h->plan.T; v.G = h->G; v.rank = h->rank;
    v.L = h->L; v.invL = h->invL; v.rc2 = h->rc2;
    v.pos = h->d_pos;
    v.v = h->d_v;
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

int not_configured(ljmd_t *h, const char *who)
{
    return fail(h, LJMD_ERR_STATE, "%s: the pressure tensor is not configured (call ljmd_stress_configure first)", who);
}

// a multi-device parent: the sum of the ranks' partial words in 192 bits; the snapshot count is common to them
int multi_fetch(ljmd_t *h, const char *who, std::vector<int64_t> *sum, int64_t *n_snapshots)
{
    if (h->stress.max_snapshots == 0) return not_configured(h, who);
    const size_t words = (size_t)h->stress.snapshots * kStressWords;
    std::vector<int64_t> part;
    try {
        part.resize(words);
        if (sum) sum->assign(words, 0);
    } catch (const std::bad_alloc &) {
        return fail(h, LJMD_ERR_ALLOC, "%s: out of host memory", who);
    }
    return for_ranks(h, [&](ljmd_t *e) {
        const int rc_ = ljmd_stress_read_exact(e, sum ? part.data() : nullptr, n_snapshots);
        for (size_t k = 0; rc_ == LJMD_OK && sum && k < words; k += 3) {
            uint64_t a[3] = {(uint64_t)(*sum)[k], (uint64_t)(*sum)[k + 1], (uint64_t)(*sum)[k + 2]};
            const uint64_t b[3] = {(uint64_t)part[k], (uint64_t)part[k + 1], (uint64_t)part[k + 2]};
            ljmdk::add192(a, b);
            for (int w = 0; w < 3; ++w) (*sum)[k + w] = (int64_t)a[w];
        }
        return rc_;
    });
}

}  // namespace

extern "C" {

int ljmd_stress_configure(ljmd_t *h, int32_t max_snapshots)
{
    static const char *who = "ljmd_stress_configure";
    LJMD_TRY(entry_checks(h, who, kHandle));
    if (h->multi) {
        // every rank runs the same guards on the same arguments: a failed guard stops at rank 0 with nothing changed
        const int rc_ = for_ranks(h, [&](ljmd_t *e) { return ljmd_stress_configure(e, max_snapshots); });
        if (rc_ == LJMD_ERR_INVALID_ARG) return rc_;
        if (rc_ != LJMD_OK) {                       // off everywhere; the first failure's message stays
            const std::string msg = h->err;
            (void)for_ranks(h, [](ljmd_t *e) { return ljmd_stress_configure(e, 0); });
            h->err = msg;
        }
        h->stress.max_snapshots = rc_ == LJMD_OK ? max_snapshots : 0;
        h->stress.snapshots = 0;
        return rc_;
    }
    LJMD_HIP(h, hipSetDevice(h->device));
    return ljmds::stress_configure(&h->stress, &h->err, who, view_of(h), max_snapshots);
}

int ljmd_stress_accumulate(ljmd_t *h)
{
    static const char *who = "ljmd_stress_accumulate";
    LJMD_TRY(entry_checks(h, who, kHandle));
    if (h->stress.max_snapshots == 0) return not_configured(h, who);
    LJMD_TRY(entry_checks(h, who, kHaveState | kHaveAccel | kNotPoisoned));
    if (h->multi) {
        // a full series stops here, before any rank has launched anything
        if (h->stress.snapshots >= h->stress.max_snapshots)
            return fail(h, LJMD_ERR_STATE, "%s: the series is full (%d snapshots; read it, then ljmd_stress_reset)", who,
                        h->stress.max_snapshots);
        LJMD_TRY(for_ranks(h, [](ljmd_t *e) { return ljmd_stress_accumulate(e); }));
        ++h->stress.snapshots;
        return LJMD_OK;
    }
    // between ljmd_step_begin and ljmd_step_finish the own block is a step ahead of the other ranks' blocks
    if (h->step_open || h->forces_pending)
        return fail(h, LJMD_ERR_STATE, "%s: inside a split-phase step (call ljmd_step_finish first)", who);
    LJMD_HIP(h, hipSetDevice(h->device));
    return ljmds::stress_accumulate(&h->stress, &h->err, who, view_of(h));
}

int ljmd_stress_read_exact(ljmd_t *h, int64_t *words, int64_t *n_snapshots)
{
    static const char *who = "ljmd_stress_read_exact";
    LJMD_TRY(entry_checks(h, who, kHandle));
    if (!h->multi) {
        LJMD_HIP(h, hipSetDevice(h->device));
        return ljmds::stress_fetch(&h->stress, &h->err, who, view_of(h), words, n_snapshots);
    }
    std::vector<int64_t> sum;
    LJMD_TRY(multi_fetch(h, who, words ? &sum : nullptr, n_snapshots));
    if (words) std::copy(sum.begin(), sum.end(), words);
    return LJMD_OK;
}

int ljmd_stress_read(ljmd_t *h, double *p, int64_t *n_snapshots)
{
    static const char *who = "ljmd_stress_read";
    LJMD_TRY(entry_checks(h, who, kHandle));
    if (!h->multi) {
        if (h->stress.max_snapshots == 0) return not_configured(h, who);
        if (h->G != 1)
            return fail(h, LJMD_ERR_STATE, "%s: a rank engine holds a partial sum (rank %d of %d): add the words of "
                                           "ljmd_stress_read_exact over the ranks and call ljmd_stress_from_exact", who, h->rank,
                        h->G);
        LJMD_HIP(h, hipSetDevice(h->device));
        return ljmds::stress_read(&h->stress, &h->err, who, view_of(h), p, n_snapshots);
    }
    std::vector<int64_t> sum;
    LJMD_TRY(multi_fetch(h, who, p ? &sum : nullptr, n_snapshots));
    for (int64_t s = 0; p && s < h->stress.snapshots; ++s)
        ljmds::stress_doubles(sum.data() + (size_t)s * kStressWords, h->L, p + (size_t)s * ljmds::kStressComponents);
    return LJMD_OK;
}

int ljmd_stress_reset(ljmd_t *h)
{
    static const char *who = "ljmd_stress_reset";
    LJMD_TRY(entry_checks(h, who, kHandle));
    if (h->multi) {
        if (h->stress.max_snapshots == 0) return not_configured(h, who);
        LJMD_TRY(for_ranks(h, [](ljmd_t *e) { return ljmd_stress_reset(e); }));
        h->stress.snapshots = 0;
        return LJMD_OK;
    }
    LJMD_HIP(h, hipSetDevice(h->device));
    return ljmds::stress_reset(&h->stress, &h->err, who, view_of(h));
}

int ljmd_stress_profile_read(ljmd_t *h, int64_t *tile_pairs_visited, int64_t *tile_pairs_total, double *kernel_ms)
{
    static const char *who = "ljmd_stress_profile_read";
    LJMD_TRY(entry_checks(h, who, kHandle));
    if (!h->multi) {
        LJMD_HIP(h, hipSetDevice(h->device));
        return ljmds::stress_profile_read(&h->stress, &h->err, who, view_of(h), tile_pairs_visited, tile_pairs_total, kernel_ms);
    }
    if (h->stress.max_snapshots == 0) return not_configured(h, who);
    // tile pairs: sums over the ranks; time: the slowest rank
    int64_t vis = 0, tot = 0;
    double ms = 0.0;
    const int rc_ = for_ranks(h, [&](ljmd_t *e) {
        int64_t a = 0, b = 0;
        double t = 0.0;
        const int r = ljmd_stress_profile_read(e, &a, &b, &t);
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

#endif  // LJMD_STRESS_CORE_ONLY
