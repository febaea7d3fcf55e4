// ljmd_origins.cpp -- the one host core of the engine's resident time-origin observables, MSD / VACF (ljmd_tcf.cpp) and
// the van Hove self-correlation (ljmd_vanhove.cpp): guards, sizes, slices, buffers, the arguments of the gather and the
// fold, reads and resets, driven by the observable's OriginDesc (ljmd_resident.h).  The core sees an engine only through
// ResidentView, references no launcher, and links without anything of struct ljmd (tests/tcf_host, tests/vanhove_host).
#include "ljmd_resident.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <new>

namespace ljmdh {

namespace {

// the buffers of a state in the order they are allocated, from the histogram on or, without one, from the sums on; the
// sizes and the ring's name matter to configure only
struct Buffers {
    std::array<DeviceBuffer, 7> all;
    int first;
    const DeviceBuffer *begin() const { return all.data() + first; }
    const DeviceBuffer *end() const { return all.data() + all.size(); }
};

Buffers buffers(OriginState *st, bool histogram, const OriginSizes &z = {}, const char *ring = "")
{
    return {{{{(void **)&st->d_hist, z.hist_bytes, "the histogram"},
              {(void **)&st->d_sums, z.sums_bytes, "the sums"},
              {(void **)&st->d_range, sizeof(int32_t), "the range word"},
              {(void **)&st->d_cur, z.cur_bytes, "the current snapshot"},
              {(void **)&st->d_part, z.part_bytes, "the partial sums"},
              {(void **)&st->d_flag, z.flag_bytes, "the range flags"},
              {(void **)&st->d_ring, z.ring_bytes, ring}}},
            histogram ? 0 : 1};
}

}  // namespace

int origin_not_configured(const OriginDesc &d, std::string *err, const char *who)
{
    return fail(err, LJMD_ERR_STATE, "%s: %s is not configured (call ljmd_%s_configure first)", who, d.phrase, d.tag);
}

OriginSizes origin_sizes(const OriginDesc &d, int n, int max_lag, int stride, int nbins)
{
    const size_t C = (size_t)d.components;
    OriginSizes z;
    z.slots = max_lag / stride + 1;
    z.ents = z.slots + 1;
    z.n_pad = ((size_t)n + ljmdk::kOriginBlock - 1) / ljmdk::kOriginBlock * ljmdk::kOriginBlock;
    z.nblk = (int)(z.n_pad / ljmdk::kOriginBlock);
    z.cur_bytes = C * z.n_pad * sizeof(double);
    z.ring_bytes = (size_t)z.slots * C * z.n_pad * sizeof(double);
    z.part_bytes = (size_t)z.nblk * (size_t)z.ents * 4 * sizeof(unsigned long long);
    z.flag_bytes = (size_t)z.nblk * (size_t)z.slots * sizeof(int32_t);
    z.sums_bytes = 2 * ((size_t)max_lag + 1) * 3 * sizeof(uint64_t);
    if (d.max_bins) z.hist_bytes = ((size_t)max_lag + 1) * ((size_t)nbins + 1) * sizeof(unsigned long long);
    return z;
}

OriginSlices origin_plan_slices(int nblk, int n_live, std::optional<int> chunk)
{
    const int want = (ljmdk::kOriginTargetWorkgroups + nblk - 1) / nblk;           // slices that fill the grid ...
    const int need = (n_live + ljmdk::kOriginMaxChunk - 1) / ljmdk::kOriginMaxChunk;   // ... and slices the LDS budget asks for
    const int slices = std::min(n_live, std::max(want, need));
    OriginSlices p;
    p.chunk = (n_live + slices - 1) / slices;
    if (chunk) p.chunk = std::max(1, std::min(*chunk, std::min(n_live, ljmdk::kOriginMaxChunk)));
    p.slices = (n_live + p.chunk - 1) / p.chunk;
    return p;
}

void origin_release(OriginState *st, hipStream_t stream)
{
    free_buffers(buffers(st, true), stream);       // a pointer that was never allocated is NULL
    st->timer.destroy();
    *st = {};
}

void origin_new_trajectory(OriginState *st) { st->s = 0; }      // the window of a snapshot follows from s: no origin is live

int origin_configure(const OriginDesc &d, OriginState *st, std::string *err, const char *who, const ResidentView &v,
                     int32_t max_lag, int32_t origin_stride, int32_t nbins, double rmax)
{
    if (max_lag < 0 || max_lag > d.max_lag)
        return fail(err, LJMD_ERR_INVALID_ARG, "%s: max_lag = %d outside 1..%d (0 switches %s off)", who, max_lag, d.max_lag,
                    d.phrase);
    if (max_lag > 0 && origin_stride < 1) return fail(err, LJMD_ERR_INVALID_ARG, "%s: origin_stride must be >= 1", who);
    if (max_lag > 0 && max_lag / origin_stride + 1 > d.max_origins)
        return fail(err, LJMD_ERR_INVALID_ARG, "%s: max_lag / origin_stride + 1 = %d exceeds LJMD_%s_MAX_ORIGINS (%d)", who,
                    max_lag / origin_stride + 1, d.limits, d.max_origins);
    if (d.max_bins && max_lag > 0 && (nbins < 1 || nbins > d.max_bins))
        return fail(err, LJMD_ERR_INVALID_ARG, "%s: nbins = %d outside 1..%d", who, nbins, d.max_bins);
    // dr = rmax / nbins and its reciprocal must be usable numbers too: a subnormal rmax is refused with the rest
    if (d.max_bins && max_lag > 0 &&
        !(std::isfinite(rmax) && rmax > 0.0 && std::isnormal(rmax / nbins) && std::isfinite(1.0 / (rmax / nbins))))
        return fail(err, LJMD_ERR_INVALID_ARG, "%s: rmax must be finite and > 0 (and rmax / nbins a normal number)", who);
    if (max_lag > 0 && (v.multi || v.G != 1))
        return fail(err, LJMD_ERR_INVALID_ARG, "%s: n_ranks = %d%s: %s of the resident system needs a one-rank engine "
                                               "(ljmd_create with n_ranks = 1)", who, v.G,
                    v.multi ? " (multi-device handle)" : "", d.phrase);
    if (max_lag > 0 && (v.n < 1 || (size_t)v.n > d.max_n || v.P < v.n))
        return fail(err, LJMD_ERR_INVALID_ARG, "%s: n = %d outside 1..%zu", who, v.n, d.max_n);
    origin_release(st, v.stream);
    if (max_lag == 0) return LJMD_OK;
    const OriginSizes z = origin_sizes(d, v.n, max_lag, origin_stride, nbins);
    char ring[48];
    std::snprintf(ring, sizeof ring, "the origin ring (%d slots)", z.slots);
    const Buffers bufs = buffers(st, d.max_bins != 0, z, ring);
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
        origin_release(st, v.stream);
        return rc_;
    }
    st->max_lag = max_lag;
    st->stride = origin_stride;
    st->n = v.n;
    if (d.max_bins) {
        st->nbins = nbins;
        st->rmax = rmax;
        st->dr = rmax / nbins;
        st->inv_dr = 1.0 / st->dr;
    }
    st->sz = z;
    return LJMD_OK;
}

int origin_accumulate(const OriginDesc &d, OriginState *st, std::string *err, const char *who, const ResidentView &v)
{
    if (st->max_lag == 0) return origin_not_configured(d, err, who);
    if (v.n != st->n || !v.ru || (d.needs_v && !v.v) || !v.perm)
        return fail(err, LJMD_ERR_STATE, "%s: the engine is not the one %s was configured for", who, d.phrase);
    const TcfWindow w = tcf_window(st->s, st->max_lag, st->stride, st->sz.slots);
    OriginSlices p;
    if (w.n_live > 0) p = origin_plan_slices(st->sz.nblk, w.n_live, d.chunk_override ? v.vanhove_chunk : std::nullopt);
    ljmdk::OriginGatherArgs ga{};
    ga.ru = v.ru; ga.v = d.needs_v ? v.v : nullptr; ga.perm = v.perm;
    ga.cur = st->d_cur;
    ga.store = w.store_slot >= 0 ? st->d_ring + (size_t)w.store_slot * d.components * st->sz.n_pad : nullptr;
    ga.n = v.n; ga.P = v.P; ga.n_pad = st->sz.n_pad;
    ljmdk::OriginFoldArgs fa{};
    fa.part = st->d_part; fa.flag = st->d_flag; fa.sums = st->d_sums; fa.range = st->d_range;
    fa.nblk = st->sz.nblk; fa.slots = st->sz.slots; fa.ents = st->sz.ents; fa.stride = st->stride; fa.max_lag = st->max_lag;
    fa.n_live = w.n_live; fa.lag_first = w.lag_first;
    fa.chunk = p.chunk; fa.slices = p.slices;
    LJMD_HIP(err, st->timer.start(v.stream));
    const hipError_t e = d.launch(*st, v, w, p, ga, fa);
    if (e != hipSuccess) return fail(err, LJMD_ERR_HIP, "%s: %s launch failed: %s", who, d.brief, hipGetErrorString(e));
    LJMD_HIP(err, st->timer.stop(v.stream));
    st->last_live = w.n_live;
    tcf_count(w, st->stride, st->counts.data());
    ++st->s;
    ++st->snapshots;
    return LJMD_OK;
}

int origin_fetch(const OriginDesc &d, OriginState *st, std::string *err, const char *who, const ResidentView &v, uint64_t *hist,
                 uint64_t *words, int64_t *counts, int64_t *n_snapshots)
{
    if (st->max_lag == 0) return origin_not_configured(d, err, who);
    static_assert(sizeof(uint64_t) == sizeof(unsigned long long), "histogram word");
    int32_t range = 0;
    LJMD_HIP(err, hipMemcpyAsync(&range, st->d_range, sizeof range, hipMemcpyDeviceToHost, v.stream));
    if (hist && st->d_hist) LJMD_HIP(err, hipMemcpyAsync(hist, st->d_hist, st->sz.hist_bytes, hipMemcpyDeviceToHost, v.stream));
    if (words) LJMD_HIP(err, hipMemcpyAsync(words, st->d_sums, st->sz.sums_bytes, hipMemcpyDeviceToHost, v.stream));
    LJMD_HIP(err, hipStreamSynchronize(v.stream));
    // the handle is not poisoned: the trajectory itself is sound
    if (range != 0) return fail(err, LJMD_ERR_RANGE, "%s: %s; the flag stays until ljmd_%s_reset", who, d.range, d.tag);
    if (counts) std::copy(st->counts.begin(), st->counts.end(), counts);
    if (n_snapshots) *n_snapshots = st->snapshots;
    return LJMD_OK;
}

int origin_read(const OriginDesc &d, OriginState *st, std::string *err, const char *who, const ResidentView &v, uint64_t *hist,
                double *kind0, double *kind1, int64_t *counts, int64_t *n_snapshots)
{
    if (st->max_lag == 0) return origin_not_configured(d, err, who);
    std::vector<uint64_t> w;
    if (kind0 || kind1) {
        try {
            w.resize(st->sz.sums_bytes / sizeof(uint64_t));
        } catch (const std::bad_alloc &) {
            return fail(err, LJMD_ERR_ALLOC, "%s: out of host memory", who);
        }
    }
    LJMD_TRY(origin_fetch(d, st, err, who, v, hist, w.empty() ? nullptr : w.data(), counts, n_snapshots));
    const size_t rows = (size_t)st->max_lag + 1;
    double *const dst[2] = {kind0, kind1};
    for (int kind = 0; kind < 2; ++kind)
        for (size_t l = 0; dst[kind] && l < rows; ++l) {
            const uint64_t *x = w.data() + ((size_t)kind * rows + l) * 3;
            const uint64_t x3[3] = {x[0], x[1], x[2]};
            dst[kind][l] = tcf_quotient(x3, st->n, st->counts[l]);       // what ljmd_tcf_from_exact computes
        }
    return LJMD_OK;
}

int origin_reset(const OriginDesc &d, OriginState *st, std::string *err, const char *who, const ResidentView &v)
{
    if (st->max_lag == 0) return origin_not_configured(d, err, who);
    if (st->d_hist) LJMD_HIP(err, hipMemsetAsync(st->d_hist, 0, st->sz.hist_bytes, v.stream));
    LJMD_HIP(err, hipMemsetAsync(st->d_sums, 0, st->sz.sums_bytes, v.stream));
    LJMD_HIP(err, hipMemsetAsync(st->d_range, 0, sizeof(int32_t), v.stream));
    std::fill(st->counts.begin(), st->counts.end(), 0);
    st->s = 0;
    st->snapshots = 0;
    return LJMD_OK;
}

int origin_profile_read(const OriginDesc &d, OriginState *st, std::string *err, const char *who, const ResidentView &v,
                        double *kernel_ms, int32_t *origins_live)
{
    if (st->max_lag == 0) return origin_not_configured(d, err, who);
    float ms = 0.0f;
    LJMD_HIP(err, st->timer.elapsed_ms(v.stream, &ms));
    if (kernel_ms) *kernel_ms = (double)ms;
    if (origins_live) *origins_live = st->timer.timed ? st->last_live : 0;
    return LJMD_OK;
}

}  // namespace ljmdh
