// ljmd_current.cpp -- the engine's resident current modes on the host (kernels: ljmd_current.hip): guards, sizes,
// buffers, the two launches of one accumulate, reads and resets.  A core beside that of the density modes
// (ljmd_rhok.cpp), whose mode-list rules, grid (RhokPlan) and conversion (rhok_doubles) it takes over: a snapshot is
// n_modes rows of eighteen words, not six, and the terms kernel reads the velocities too.  Like the other cores it sees
// an engine only through ResidentView and links without anything of struct ljmd (tests/current_host); the C entry points
// that take a handle are in ljmd_resident.cpp.
#include "ljmd_resident.h"

#include <cstdlib>
#include <new>

using namespace ljmdh;

namespace ljmdc {

namespace {

static_assert(kCurrentMaxSnapshots == LJMD_CURRENT_MAX_SNAPSHOTS && kCurrentMaxEntries == LJMD_CURRENT_MAX_ENTRIES,
              "LJMD_CURRENT_* out of sync with the core");

enum { kSeries, kModes, kPart, kFlag, kRange, kBuffers };

// the buffers of a state in the order they are allocated; the sizes matter to configure only
std::array<DeviceBuffer, kBuffers> buffers(CurrentState *st, int max_snapshots = 0, int n_modes = 0, const RhokPlan &p = {})
{
    const size_t row = (size_t)kCurrentRowWords * sizeof(uint64_t);
    return {{{(void **)&st->d_series, (size_t)max_snapshots * n_modes * row, "the series"},
             {(void **)&st->d_modes, (size_t)n_modes * 3 * sizeof(int32_t), "the mode list"},
             {(void **)&st->d_part, (size_t)p.pchunks * p.mchunks * kRhokModeChunk * row, "the partials"},
             {(void **)&st->d_flag, (size_t)p.pchunks * p.mchunks * sizeof(unsigned), "the flags"},
             {(void **)&st->d_range, sizeof(int32_t), "the range word"}}};
}

size_t series_bytes(const CurrentState *st, int64_t snapshots)
{
    return (size_t)snapshots * st->n_modes * kCurrentRowWords * sizeof(uint64_t);
}

}  // namespace

int current_not_configured(std::string *err, const char *who)
{
    return fail(err, LJMD_ERR_STATE, "%s: the current modes are not configured (call ljmd_current_configure first)", who);
}

void current_release(CurrentState *st, hipStream_t stream)
{
    free_buffers(buffers(st), stream);
    st->timer.destroy();
    *st = {};
}

int current_configure(CurrentState *st, std::string *err, const char *who, const ResidentView &v, int32_t n_modes,
                      const int32_t *modes, int32_t max_snapshots)
{
    if (max_snapshots < 0 || max_snapshots > kCurrentMaxSnapshots)
        return fail(err, LJMD_ERR_INVALID_ARG, "%s: max_snapshots = %d outside 1..%d (0 switches the current modes off)", who,
                    max_snapshots, kCurrentMaxSnapshots);
    if (max_snapshots == 0) {
        current_release(st, v.stream);
        return LJMD_OK;
    }
    if (v.multi || v.G != 1)
        return fail(err, LJMD_ERR_INVALID_ARG, "%s: n_ranks = %d%s: a rank holds only its own particles and the sum runs over "
                                               "all of them, so the current modes of the resident system need a one-rank "
                                               "engine (ljmd_create with n_ranks = 1)", who, v.G,
                    v.multi ? " (multi-device handle)" : "");
    if (n_modes < 1 || n_modes > kRhokMaxModes)
        return fail(err, LJMD_ERR_INVALID_ARG, "%s: n_modes = %d outside 1..%d", who, n_modes, kRhokMaxModes);
    if (!modes) return fail(err, LJMD_ERR_INVALID_ARG, "%s: modes is NULL", who);
    for (int m = 0; m < n_modes; ++m)
        for (int a = 0; a < 3; ++a)
            if (modes[3 * m + a] < -kRhokMaxIndex || modes[3 * m + a] > kRhokMaxIndex)
                return fail(err, LJMD_ERR_INVALID_ARG, "%s: mode %d = (%d, %d, %d): an index outside -%d..%d", who, m,
                            modes[3 * m], modes[3 * m + 1], modes[3 * m + 2], kRhokMaxIndex, kRhokMaxIndex);
    if ((int64_t)max_snapshots * n_modes > kCurrentMaxEntries)
        return fail(err, LJMD_ERR_INVALID_ARG, "%s: max_snapshots * n_modes = %lld above %d", who,
                    (long long)max_snapshots * n_modes, kCurrentMaxEntries);
    if (v.n < 1 || v.n > kRhokMaxN) return fail(err, LJMD_ERR_INVALID_ARG, "%s: n = %d outside 1..%d", who, v.n, kRhokMaxN);
    current_release(st, v.stream);
    const RhokPlan p = rhok_plan(v.T, n_modes);
    const auto bufs = buffers(st, max_snapshots, n_modes, p);
    auto body = [&]() -> int {
        LJMD_TRY(alloc_buffers(err, who, bufs));
        LJMD_HIP(err, st->timer.create());
        // the partials and flags are written before they are read; the rest starts at zero
        LJMD_HIP(err, hipMemsetAsync(st->d_series, 0, bufs[kSeries].bytes, v.stream));
        LJMD_HIP(err, hipMemsetAsync(st->d_range, 0, bufs[kRange].bytes, v.stream));
        LJMD_HIP(err, hipMemcpyAsync(st->d_modes, modes, bufs[kModes].bytes, hipMemcpyHostToDevice, v.stream));
        LJMD_HIP(err, hipStreamSynchronize(v.stream));      // the caller's list is free again
        return LJMD_OK;
    };
    const int rc_ = body();
    if (rc_ != LJMD_OK) {
        current_release(st, v.stream);
        return rc_;
    }
    st->max_snapshots = max_snapshots;
    st->n_modes = n_modes;
    st->n = v.n;
    st->T = v.T;
    st->plan = p;
    return LJMD_OK;
}

int current_accumulate(CurrentState *st, std::string *err, const char *who, const ResidentView &v)
{
    if (st->max_snapshots == 0) return current_not_configured(err, who);
    if (st->snapshots >= st->max_snapshots)
        return fail(err, LJMD_ERR_STATE, "%s: the series is full (%d snapshots; read it, then ljmd_current_reset)", who,
                    st->max_snapshots);
    if (v.G != 1 || v.multi || v.T != st->T || v.n != st->n || !v.pos || !v.v || !v.perm)
        return fail(err, LJMD_ERR_STATE, "%s: the engine is not the one the current modes were configured for", who);
    CurrentTermsArgs ta{};
    ta.pos = v.pos; ta.v = v.v; ta.perm = v.perm; ta.modes = st->d_modes;
    ta.part = st->d_part; ta.flag = st->d_flag;
    ta.P = v.P; ta.T = v.T; ta.n = v.n; ta.n_modes = st->n_modes;
    ta.mchunks = st->plan.mchunks; ta.pchunks = st->plan.pchunks; ta.tiles = st->plan.tiles;
    ta.L = v.L;
    CurrentFoldArgs fa{};
    fa.part = st->d_part; fa.flag = st->d_flag;
    fa.n_modes = st->n_modes; fa.mchunks = st->plan.mchunks; fa.pchunks = st->plan.pchunks;
    fa.row = st->d_series + (size_t)st->snapshots * st->n_modes * kCurrentRowWords;
    fa.range = st->d_range;
    LJMD_HIP(err, st->timer.start(v.stream));
    hipError_t e = launch_current_terms(ta, v.stream);
    if (e == hipSuccess) e = launch_current_fold(fa, v.stream);
    if (e != hipSuccess) return fail(err, LJMD_ERR_HIP, "%s: current modes launch failed: %s", who, hipGetErrorString(e));
    LJMD_HIP(err, st->timer.stop(v.stream));
    ++st->snapshots;
    return LJMD_OK;
}

int current_fetch(CurrentState *st, std::string *err, const char *who, const ResidentView &v, int64_t *words,
                  int64_t *n_snapshots)
{
    if (st->max_snapshots == 0) return current_not_configured(err, who);
    int32_t range = 0;
    LJMD_HIP(err, hipMemcpyAsync(&range, st->d_range, sizeof range, hipMemcpyDeviceToHost, v.stream));
    if (words && st->snapshots > 0)
        LJMD_HIP(err, hipMemcpyAsync(words, st->d_series, series_bytes(st, st->snapshots), hipMemcpyDeviceToHost, v.stream));
    LJMD_HIP(err, hipStreamSynchronize(v.stream));
    // the handle is not poisoned: the trajectory itself is sound
    if (range != 0)
        return fail(err, LJMD_ERR_RANGE, "%s: a particle's current mode terms were not finite or reached 2^40 (a coordinate, "
                                         "a velocity or the box length) and entered as 0; the flag stays until "
                                         "ljmd_current_reset", who);
    if (n_snapshots) *n_snapshots = st->snapshots;
    return LJMD_OK;
}

int current_read(CurrentState *st, std::string *err, const char *who, const ResidentView &v, double *j, int64_t *n_snapshots)
{
    if (st->max_snapshots == 0) return current_not_configured(err, who);
    std::vector<int64_t> w;
    if (j) {
        try {
            w.resize((size_t)st->snapshots * st->n_modes * kCurrentRowWords);
        } catch (const std::bad_alloc &) {
            return fail(err, LJMD_ERR_ALLOC, "%s: out of host memory", who);
        }
    }
    LJMD_TRY(current_fetch(st, err, who, v, j ? w.data() : nullptr, n_snapshots));
    if (j) rhok_doubles(w.data(), w.size() / 3, j);
    return LJMD_OK;
}

int current_reset(CurrentState *st, std::string *err, const char *who, const ResidentView &v)
{
    if (st->max_snapshots == 0) return current_not_configured(err, who);
    LJMD_HIP(err, hipMemsetAsync(st->d_series, 0, series_bytes(st, st->max_snapshots), v.stream));
    LJMD_HIP(err, hipMemsetAsync(st->d_range, 0, sizeof(int32_t), v.stream));
    st->snapshots = 0;
    return LJMD_OK;
}

int current_profile_read(CurrentState *st, std::string *err, const char *who, const ResidentView &v, double *kernel_ms)
{
    if (st->max_snapshots == 0) return current_not_configured(err, who);
    float ms = 0.0f;
    LJMD_HIP(err, st->timer.elapsed_ms(v.stream, &ms));
    if (kernel_ms) *kernel_ms = (double)ms;
    return LJMD_OK;
}

}  // namespace ljmdc
