// ljmd_rhok.cpp -- the engine's resident density modes on the host (kernels: ljmd_rhok.hip): guards, sizes, buffers, the
// two launches of one accumulate, reads and resets, and ljmd_rhok_select_modes, which needs no engine.  A core of its
// own beside the series core (ljmd_series.cpp): a snapshot here has a run-time word count, a mode list on the device and
// no pair part -- no tile boxes, no walk plan, no tile-pair counts -- so that SeriesDesc would share little more than the
// guards.  Like the other cores it sees an engine only through ResidentView and links without anything of struct ljmd
// (tests/rhok_host); the C entry points that take a handle are in ljmd_resident.cpp.
#include "ljmd_resident.h"

#include <cstdlib>
#include <new>

using namespace ljmdh;

namespace ljmdc {

namespace {

static_assert(kRhokMaxModes == LJMD_RHOK_MAX_MODES && kRhokMaxIndex == LJMD_RHOK_MAX_INDEX &&
                  kRhokMaxSnapshots == LJMD_RHOK_MAX_SNAPSHOTS && kRhokMaxEntries == LJMD_RHOK_MAX_ENTRIES,
              "LJMD_RHOK_* out of sync with the core");

enum { kSeries, kModes, kPart, kFlag, kRange, kBuffers };

// the buffers of a state in the order they are allocated; the sizes matter to configure only
std::array<DeviceBuffer, kBuffers> buffers(RhokState *st, int max_snapshots = 0, int n_modes = 0, const RhokPlan &p = {})
{
    const size_t row = (size_t)kRhokRowWords * sizeof(uint64_t);
    return {{{(void **)&st->d_series, (size_t)max_snapshots * n_modes * row, "the series"},
             {(void **)&st->d_modes, (size_t)n_modes * 3 * sizeof(int32_t), "the mode list"},
             {(void **)&st->d_part, (size_t)p.pchunks * p.mchunks * kRhokModeChunk * row, "the partials"},
             {(void **)&st->d_flag, (size_t)p.pchunks * p.mchunks * sizeof(unsigned), "the flags"},
             {(void **)&st->d_range, sizeof(int32_t), "the range word"}}};
}

size_t series_bytes(const RhokState *st, int64_t snapshots)
{
    return (size_t)snapshots * st->n_modes * kRhokRowWords * sizeof(uint64_t);
}

}  // namespace

int not_configured(std::string *err, const char *who)
{
    return fail(err, LJMD_ERR_STATE, "%s: the density modes are not configured (call ljmd_rhok_configure first)", who);
}

void rhok_release(RhokState *st, hipStream_t stream)
{
    free_buffers(buffers(st), stream);
    st->timer.destroy();
    *st = {};
}

int rhok_configure(RhokState *st, std::string *err, const char *who, const ResidentView &v, int32_t n_modes,
                   const int32_t *modes, int32_t max_snapshots)
{
    if (max_snapshots < 0 || max_snapshots > kRhokMaxSnapshots)
        return fail(err, LJMD_ERR_INVALID_ARG, "%s: max_snapshots = %d outside 1..%d (0 switches the density modes off)", who,
                    max_snapshots, kRhokMaxSnapshots);
    if (max_snapshots == 0) {
        rhok_release(st, v.stream);
        return LJMD_OK;
    }
    if (v.multi || v.G != 1)
        return fail(err, LJMD_ERR_INVALID_ARG, "%s: n_ranks = %d%s: a rank holds only its own particles and the sum runs over "
                                               "all of them, so the density modes of the resident system need a one-rank "
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
    if ((int64_t)max_snapshots * n_modes > kRhokMaxEntries)
        return fail(err, LJMD_ERR_INVALID_ARG, "%s: max_snapshots * n_modes = %lld above %d", who,
                    (long long)max_snapshots * n_modes, kRhokMaxEntries);
    if (v.n < 1 || v.n > kRhokMaxN) return fail(err, LJMD_ERR_INVALID_ARG, "%s: n = %d outside 1..%d", who, v.n, kRhokMaxN);
    rhok_release(st, v.stream);
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
        rhok_release(st, v.stream);
        return rc_;
    }
    st->max_snapshots = max_snapshots;
    st->n_modes = n_modes;
    st->n = v.n;
    st->T = v.T;
    st->plan = p;
    return LJMD_OK;
}

int rhok_accumulate(RhokState *st, std::string *err, const char *who, const ResidentView &v)
{
    if (st->max_snapshots == 0) return not_configured(err, who);
    if (st->snapshots >= st->max_snapshots)
        return fail(err, LJMD_ERR_STATE, "%s: the series is full (%d snapshots; read it, then ljmd_rhok_reset)", who,
                    st->max_snapshots);
    if (v.G != 1 || v.multi || v.T != st->T || v.n != st->n || !v.pos || !v.perm)
        return fail(err, LJMD_ERR_STATE, "%s: the engine is not the one the density modes were configured for", who);
    RhokTermsArgs ta{};
    ta.pos = v.pos; ta.perm = v.perm; ta.modes = st->d_modes;
    ta.part = st->d_part; ta.flag = st->d_flag;
    ta.P = v.P; ta.T = v.T; ta.n = v.n; ta.n_modes = st->n_modes;
    ta.mchunks = st->plan.mchunks; ta.pchunks = st->plan.pchunks; ta.tiles = st->plan.tiles;
    ta.L = v.L;
    RhokFoldArgs fa{};
    fa.part = st->d_part; fa.flag = st->d_flag;
    fa.n_modes = st->n_modes; fa.mchunks = st->plan.mchunks; fa.pchunks = st->plan.pchunks;
    fa.row = st->d_series + (size_t)st->snapshots * st->n_modes * kRhokRowWords;
    fa.range = st->d_range;
    LJMD_HIP(err, st->timer.start(v.stream));
    hipError_t e = launch_rhok_terms(ta, v.stream);
    if (e == hipSuccess) e = launch_rhok_fold(fa, v.stream);
    if (e != hipSuccess) return fail(err, LJMD_ERR_HIP, "%s: density modes launch failed: %s", who, hipGetErrorString(e));
    LJMD_HIP(err, st->timer.stop(v.stream));
    ++st->snapshots;
    return LJMD_OK;
}

int rhok_fetch(RhokState *st, std::string *err, const char *who, const ResidentView &v, int64_t *words, int64_t *n_snapshots)
{
    if (st->max_snapshots == 0) return not_configured(err, who);
    int32_t range = 0;
    LJMD_HIP(err, hipMemcpyAsync(&range, st->d_range, sizeof range, hipMemcpyDeviceToHost, v.stream));
    if (words && st->snapshots > 0)
        LJMD_HIP(err, hipMemcpyAsync(words, st->d_series, series_bytes(st, st->snapshots), hipMemcpyDeviceToHost, v.stream));
    LJMD_HIP(err, hipStreamSynchronize(v.stream));
    // the handle is not poisoned: the trajectory itself is sound
    if (range != 0)
        return fail(err, LJMD_ERR_RANGE, "%s: a particle's density mode terms were not finite (a coordinate or the box "
                                         "length is not) and entered as 0; the flag stays until ljmd_rhok_reset", who);
    if (n_snapshots) *n_snapshots = st->snapshots;
    return LJMD_OK;
}

int rhok_read(RhokState *st, std::string *err, const char *who, const ResidentView &v, double *rho, int64_t *n_snapshots)
{
    if (st->max_snapshots == 0) return not_configured(err, who);
    std::vector<int64_t> w;
    if (rho) {
        try {
            w.resize((size_t)st->snapshots * st->n_modes * kRhokRowWords);
        } catch (const std::bad_alloc &) {
            return fail(err, LJMD_ERR_ALLOC, "%s: out of host memory", who);
        }
    }
    LJMD_TRY(rhok_fetch(st, err, who, v, rho ? w.data() : nullptr, n_snapshots));
    if (rho) rhok_doubles(w.data(), w.size() / 3, rho);
    return LJMD_OK;
}

int rhok_reset(RhokState *st, std::string *err, const char *who, const ResidentView &v)
{
    if (st->max_snapshots == 0) return not_configured(err, who);
    LJMD_HIP(err, hipMemsetAsync(st->d_series, 0, series_bytes(st, st->max_snapshots), v.stream));
    LJMD_HIP(err, hipMemsetAsync(st->d_range, 0, sizeof(int32_t), v.stream));
    st->snapshots = 0;
    return LJMD_OK;
}

int rhok_profile_read(RhokState *st, std::string *err, const char *who, const ResidentView &v, double *kernel_ms)
{
    if (st->max_snapshots == 0) return not_configured(err, who);
    float ms = 0.0f;
    LJMD_HIP(err, st->timer.elapsed_ms(v.stream, &ms));
    if (kernel_ms) *kernel_ms = (double)ms;
    return LJMD_OK;
}

}  // namespace ljmdc

// the triples of the half-space with 1 <= |n|^2 <= n2_max, by |n|^2 ascending and lexicographic within a shell; a shell
// of count > per_shell members keeps those at floor(j count / per_shell), j = 0 .. per_shell - 1
extern "C" int ljmd_rhok_select_modes(int32_t n2_max, int32_t per_shell, int32_t capacity, int32_t *modes, int32_t *n_modes)
{
    static const char *who = "ljmd_rhok_select_modes";
    const int64_t lim = (int64_t)LJMD_RHOK_MAX_INDEX * LJMD_RHOK_MAX_INDEX;
    if (n2_max < 1 || n2_max > lim)
        return fail(nullptr, LJMD_ERR_INVALID_ARG, "%s: n2_max = %d outside 1..%lld", who, n2_max, (long long)lim);
    if (per_shell < 1) return fail(nullptr, LJMD_ERR_INVALID_ARG, "%s: per_shell = %d must be >= 1", who, per_shell);
    if (capacity < 0 || !n_modes || (capacity > 0 && !modes))
        return fail(nullptr, LJMD_ERR_INVALID_ARG, "%s: NULL argument or capacity < 0", who);
    int r = 0;
    while ((int64_t)(r + 1) * (r + 1) <= n2_max) ++r;
    // two walks over the half-space in lexicographic order: the members of every shell, then each member to its place
    std::vector<int64_t> count, first, seen;        // per |n|^2: members, index of the shell's first kept mode, members met
    try {
        count.assign((size_t)n2_max + 1, 0);
        first.assign((size_t)n2_max + 2, 0);
        seen.assign((size_t)n2_max + 1, 0);
    } catch (const std::bad_alloc &) {
        return fail(nullptr, LJMD_ERR_ALLOC, "%s: out of host memory", who);
    }
    auto walk = [&](auto &&visit) {
        for (int x = 0; x <= r; ++x)
            for (int y = (x > 0 ? -r : 0); y <= r; ++y) {
                const int64_t xy = (int64_t)x * x + (int64_t)y * y;
                // the half-space: the first non-zero index is positive
                for (int z = (x > 0 || y > 0 ? -r : 1); z <= r; ++z) {
                    const int64_t n2 = xy + (int64_t)z * z;
                    if (n2 >= 1 && n2 <= n2_max) visit(n2, x, y, z);
                }
            }
    };
    walk([&](int64_t n2, int, int, int) { ++count[(size_t)n2]; });
    for (int64_t n2 = 1; n2 <= n2_max; ++n2)
        first[(size_t)n2 + 1] = first[(size_t)n2] + std::min<int64_t>(count[(size_t)n2], per_shell);
    const int64_t total = first[(size_t)n2_max + 1];
    walk([&](int64_t n2, int x, int y, int z) {
        const int64_t c = count[(size_t)n2], k = seen[(size_t)n2]++;
        // member k is kept when k = floor(j c / per_shell) for a j < per_shell: the smallest j with j c >= k per_shell
        const int64_t j = c > per_shell ? (k * per_shell + c - 1) / c : k;
        if (j >= per_shell || (c > per_shell && j * c / per_shell != k)) return;
        const int64_t at = first[(size_t)n2] + j;
        if (at < capacity) {
            modes[3 * at] = x;
            modes[3 * at + 1] = y;
            modes[3 * at + 2] = z;
        }
    });
    if (total > INT32_MAX) return fail(nullptr, LJMD_ERR_INVALID_ARG, "%s: more than 2^31 - 1 modes", who);
    *n_modes = (int32_t)total;
    if (total > capacity)
        return fail(nullptr, LJMD_ERR_INVALID_ARG, "%s: capacity = %d too small: %lld modes", who, capacity, (long long)total);
    return LJMD_OK;
}
