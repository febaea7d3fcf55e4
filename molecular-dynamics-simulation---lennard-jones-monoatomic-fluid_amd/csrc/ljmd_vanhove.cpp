// ljmd_vanhove.cpp -- host core of the van Hove self-correlation of the system resident on a one-rank engine (kernels:
// ljmd_vanhove.hip): guards, sizes, argument blocks, launches, reads and resets.  Snapshot numbering, window, counts and
// quotient are the MSD / VACF accumulation's own (ljmd_tcf_host.h).  It sees an engine only through ResidentView and
// links without anything of struct ljmd (tests/vanhove_host); the C entry points are in ljmd_resident.cpp.
#include "ljmd_resident.h"
#include "ljmd_tcf_host.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <new>

using namespace ljmdh;

namespace ljmdv {

namespace {

// the buffers of a state in the order they are allocated; the sizes and the ring's name matter to configure only
std::array<DeviceBuffer, 7> buffers(VanHoveState *st, const VhSizes &z = {}, const char *ring = "")
{
    return {{{(void **)&st->d_hist, z.hist_bytes, "the histogram"},
             {(void **)&st->d_sums, z.sums_bytes, "the sums"},
             {(void **)&st->d_range, sizeof(int32_t), "the range word"},
             {(void **)&st->d_cur, z.cur_bytes, "the current snapshot"},
             {(void **)&st->d_part, z.part_bytes, "the partial sums"},
             {(void **)&st->d_flag, z.flag_bytes, "the range flags"},
             {(void **)&st->d_ring, z.ring_bytes, ring}}};
}

}  // namespace

int not_configured(std::string *err, const char *who)
{
    return fail(err, LJMD_ERR_STATE, "%s: the van Hove function is not configured (call ljmd_vanhove_configure first)", who);
}

VhSizes vanhove_sizes(int n, int max_lag, int stride, int nbins)
{
    VhSizes z;
    z.slots = max_lag / stride + 1;
    z.ents = z.slots + 1;
    z.n_pad = ((size_t)n + kVhBlock - 1) / kVhBlock * kVhBlock;
    z.nblk = (int)(z.n_pad / kVhBlock);
    z.cur_bytes = 3 * z.n_pad * sizeof(double);
    z.ring_bytes = (size_t)z.slots * 3 * z.n_pad * sizeof(double);
    z.part_bytes = (size_t)z.nblk * (size_t)z.ents * 4 * sizeof(unsigned long long);
    z.flag_bytes = (size_t)z.nblk * (size_t)z.slots * sizeof(int32_t);
    z.sums_bytes = 2 * ((size_t)max_lag + 1) * 3 * sizeof(uint64_t);
    z.hist_bytes = ((size_t)max_lag + 1) * ((size_t)nbins + 1) * sizeof(unsigned long long);
    return z;
}

VhSlices vanhove_plan_slices(int nblk, int n_live, std::optional<int> chunk)
{
    const int want = (kVhTargetWorkgroups + nblk - 1) / nblk;                  // slices that fill the grid ...
    const int need = (n_live + kVhMaxChunk - 1) / kVhMaxChunk;                 // ... and slices the LDS budget asks for
    const int slices = std::min(n_live, std::max(want, need));
    VhSlices p;
    p.chunk = (n_live + slices - 1) / slices;
    if (chunk) p.chunk = std::max(1, std::min(*chunk, std::min(n_live, kVhMaxChunk)));
    p.slices = (n_live + p.chunk - 1) / p.chunk;
    return p;
}

void vanhove_release(VanHoveState *st, hipStream_t stream)
{
    free_buffers(buffers(st), stream);
    st->timer.destroy();
    *st = {};
}

void vanhove_new_trajectory(VanHoveState *st) { st->s = 0; }    // the window of a snapshot follows from s: no origin is live

int vanhove_configure(VanHoveState *st, std::string *err, const char *who, const ResidentView &v, int32_t max_lag,
                      int32_t origin_stride, int32_t nbins, double rmax)
{
    static_assert(kVhMaxLag == LJMD_VANHOVE_MAX_LAG && kVhMaxOrigins == LJMD_VANHOVE_MAX_ORIGINS &&
                      kVhMaxBins == LJMD_VANHOVE_MAX_BINS, "van Hove limits out of sync with include/ljmd.h");
    if (max_lag < 0 || max_lag > kVhMaxLag)
        return fail(err, LJMD_ERR_INVALID_ARG, "%s: max_lag = %d outside 1..%d (0 switches the van Hove function off)", who,
                    max_lag, kVhMaxLag);
    if (max_lag > 0 && origin_stride < 1) return fail(err, LJMD_ERR_INVALID_ARG, "%s: origin_stride must be >= 1", who);
    if (max_lag > 0 && max_lag / origin_stride + 1 > kVhMaxOrigins)
        return fail(err, LJMD_ERR_INVALID_ARG, "%s: max_lag / origin_stride + 1 = %d exceeds LJMD_VANHOVE_MAX_ORIGINS (%d)", who,
                    max_lag / origin_stride + 1, kVhMaxOrigins);
    if (max_lag > 0 && (nbins < 1 || nbins > kVhMaxBins))
        return fail(err, LJMD_ERR_INVALID_ARG, "%s: nbins = %d outside 1..%d", who, nbins, kVhMaxBins);
    // dr = rmax / nbins and its reciprocal must be usable numbers too: a subnormal rmax is refused with the rest
    if (max_lag > 0 && !(std::isfinite(rmax) && rmax > 0.0 && std::isnormal(rmax / nbins) && std::isfinite(1.0 / (rmax / nbins))))
        return fail(err, LJMD_ERR_INVALID_ARG, "%s: rmax must be finite and > 0 (and rmax / nbins a normal number)", who);
    if (max_lag > 0 && (v.multi || v.G != 1))
        return fail(err, LJMD_ERR_INVALID_ARG, "%s: n_ranks = %d%s: the van Hove function of the resident system needs a "
                                               "one-rank engine (ljmd_create with n_ranks = 1)", who, v.G,
                    v.multi ? " (multi-device handle)" : "");
    if (max_lag > 0 && (v.n < 1 || (size_t)v.n > kVhMaxN || v.P < v.n))
        return fail(err, LJMD_ERR_INVALID_ARG, "%s: n = %d outside 1..%zu", who, v.n, kVhMaxN);
    vanhove_release(st, v.stream);
    if (max_lag == 0) return LJMD_OK;
    const VhSizes z = vanhove_sizes(v.n, max_lag, origin_stride, nbins);
    char ring[48];
    std::snprintf(ring, sizeof ring, "the origin ring (%d slots)", z.slots);
    const auto bufs = buffers(st, z, ring);
    auto body = [&]() -> int {
        try {
            st->counts.assign((size_t)max_lag + 1, 0);
        } catch (const std::bad_alloc &) {
            return fail(err, LJMD_ERR_ALLOC, "%s: out of host memory for the counts", who);
        }
        LJMD_TRY(alloc_buffers(err, who, bufs));
        LJMD_HIP(err, st->timer.create());
        // the padding of cur and of the ring is zeroed here and never written; part and flag are written before read
        for (const DeviceBuffer &b : bufs) LJMD_HIP(err, hipMemsetAsync(*b.p, 0, b.bytes, v.stream));
        return LJMD_OK;
    };
    const int rc_ = body();
    if (rc_ != LJMD_OK) {
        vanhove_release(st, v.stream);
        return rc_;
    }
    st->max_lag = max_lag;
    st->stride = origin_stride;
    st->n = v.n;
    st->nbins = nbins;
    st->rmax = rmax;
    st->dr = rmax / nbins;
    st->inv_dr = 1.0 / st->dr;
    st->sz = z;
    return LJMD_OK;
}

int vanhove_accumulate(VanHoveState *st, std::string *err, const char *who, const ResidentView &v)
{
    if (st->max_lag == 0) return not_configured(err, who);
    if (v.n != st->n || !v.ru || !v.perm)
        return fail(err, LJMD_ERR_STATE, "%s: the engine is not the one the van Hove function was configured for", who);
    const TcfWindow w = tcf_window(st->s, st->max_lag, st->stride, st->sz.slots);
    VhGatherArgs ga{};
    ga.ru = v.ru; ga.perm = v.perm;
    ga.cur = st->d_cur;
    ga.store = w.store_slot >= 0 ? st->d_ring + (size_t)w.store_slot * 3 * st->sz.n_pad : nullptr;
    ga.n = v.n; ga.P = v.P; ga.n_pad = st->sz.n_pad;
    LJMD_HIP(err, st->timer.start(v.stream));
    hipError_t e = launch_vanhove_gather(ga, v.stream);
    if (e == hipSuccess && w.n_live > 0) {
        const VhSlices p = vanhove_plan_slices(st->sz.nblk, w.n_live, v.vanhove_chunk);
        VhTermsArgs ta{};
        ta.cur = st->d_cur; ta.ring = st->d_ring; ta.hist = st->d_hist; ta.part = st->d_part; ta.flag = st->d_flag;
        ta.n_pad = st->sz.n_pad;
        ta.dr = st->dr; ta.inv_dr = st->inv_dr;
        ta.n = st->n; ta.nbins = st->nbins; ta.max_lag = st->max_lag;
        ta.nblk = st->sz.nblk; ta.slots = st->sz.slots; ta.ents = st->sz.ents; ta.stride = st->stride;
        ta.n_live = w.n_live; ta.lag_first = w.lag_first; ta.slot_first = w.slot_first;
        ta.chunk = p.chunk; ta.slices = p.slices;
        VhFoldArgs fa{};
        fa.part = st->d_part; fa.flag = st->d_flag; fa.sums = st->d_sums; fa.range = st->d_range;
        fa.nblk = st->sz.nblk; fa.slots = st->sz.slots; fa.ents = st->sz.ents; fa.stride = st->stride; fa.max_lag = st->max_lag;
        fa.n_live = w.n_live; fa.lag_first = w.lag_first;
        fa.chunk = p.chunk; fa.slices = p.slices;
        e = launch_vanhove_terms(ta, v.stream);
        if (e == hipSuccess) e = launch_vanhove_fold(fa, v.stream);
    }
    if (e != hipSuccess) return fail(err, LJMD_ERR_HIP, "%s: van Hove launch failed: %s", who, hipGetErrorString(e));
    LJMD_HIP(err, st->timer.stop(v.stream));
    st->last_live = w.n_live;
    tcf_count(w, st->stride, st->counts.data());
    ++st->s;
    ++st->snapshots;
    return LJMD_OK;
}

int vanhove_fetch(VanHoveState *st, std::string *err, const char *who, const ResidentView &v, uint64_t *hist, uint64_t *words,
                  int64_t *counts, int64_t *n_snapshots)
{
    if (st->max_lag == 0) return not_configured(err, who);
    static_assert(sizeof(uint64_t) == sizeof(unsigned long long), "histogram word");
    int32_t range = 0;
    LJMD_HIP(err, hipMemcpyAsync(&range, st->d_range, sizeof range, hipMemcpyDeviceToHost, v.stream));
    if (hist) LJMD_HIP(err, hipMemcpyAsync(hist, st->d_hist, st->sz.hist_bytes, hipMemcpyDeviceToHost, v.stream));
    if (words) LJMD_HIP(err, hipMemcpyAsync(words, st->d_sums, st->sz.sums_bytes, hipMemcpyDeviceToHost, v.stream));
    LJMD_HIP(err, hipStreamSynchronize(v.stream));
    // the handle is not poisoned: the trajectory itself is sound
    if (range != 0)
        return fail(err, LJMD_ERR_RANGE, "%s: a van Hove displacement was not finite or r^4 >= 2^40: it was counted in the "
                                         "overflow column and entered the sums as 0; the flag stays until ljmd_vanhove_reset", who);
    if (counts) std::copy(st->counts.begin(), st->counts.end(), counts);
    if (n_snapshots) *n_snapshots = st->snapshots;
    return LJMD_OK;
}

int vanhove_read(VanHoveState *st, std::string *err, const char *who, const ResidentView &v, uint64_t *hist, double *r2,
                 double *r4, int64_t *counts, int64_t *n_snapshots)
{
    if (st->max_lag == 0) return not_configured(err, who);
    std::vector<uint64_t> w;
    if (r2 || r4) {
        try {
            w.resize(st->sz.sums_bytes / sizeof(uint64_t));
        } catch (const std::bad_alloc &) {
            return fail(err, LJMD_ERR_ALLOC, "%s: out of host memory", who);
        }
    }
    LJMD_TRY(vanhove_fetch(st, err, who, v, hist, w.empty() ? nullptr : w.data(), counts, n_snapshots));
    const size_t rows = (size_t)st->max_lag + 1;
    double *const dst[2] = {r2, r4};
    for (int kind = 0; kind < 2; ++kind)
        for (size_t l = 0; dst[kind] && l < rows; ++l) {
            const uint64_t *x = w.data() + ((size_t)kind * rows + l) * 3;
            const uint64_t x3[3] = {x[0], x[1], x[2]};
            dst[kind][l] = tcf_quotient(x3, st->n, st->counts[l]);       // what ljmd_tcf_from_exact computes
        }
    return LJMD_OK;
}

int vanhove_reset(VanHoveState *st, std::string *err, const char *who, const ResidentView &v)
{
    if (st->max_lag == 0) return not_configured(err, who);
    LJMD_HIP(err, hipMemsetAsync(st->d_hist, 0, st->sz.hist_bytes, v.stream));
    LJMD_HIP(err, hipMemsetAsync(st->d_sums, 0, st->sz.sums_bytes, v.stream));
    LJMD_HIP(err, hipMemsetAsync(st->d_range, 0, sizeof(int32_t), v.stream));
    std::fill(st->counts.begin(), st->counts.end(), 0);
    st->s = 0;
    st->snapshots = 0;
    return LJMD_OK;
}

int vanhove_profile_read(VanHoveState *st, std::string *err, const char *who, const ResidentView &v, double *kernel_ms,
                         int32_t *origins_live)
{
    if (st->max_lag == 0) return not_configured(err, who);
    float ms = 0.0f;
    LJMD_HIP(err, st->timer.elapsed_ms(v.stream, &ms));
    if (kernel_ms) *kernel_ms = (double)ms;
    if (origins_live) *origins_live = st->timer.timed ? st->last_live : 0;
    return LJMD_OK;
}

}  // namespace ljmdv
