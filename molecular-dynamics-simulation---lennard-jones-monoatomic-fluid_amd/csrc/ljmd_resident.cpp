// ljmd_resident.cpp -- the C entry points of the seven observables of the system resident on the single / sharded
// engine (include/ljmd.h: ljmd_rdf_*, ljmd_tcf_*, ljmd_stress_*, ljmd_heatflux_*, ljmd_vanhove_*, ljmd_rhok_*,
// ljmd_current_*) and the release of what they allocated.  Each runs the entry checks, builds the view of the engine and
// calls the observable's core (ljmd_rdf.cpp, ljmd_tcf.cpp, ljmd_stress.cpp, ljmd_heatflux.cpp, ljmd_vanhove.cpp,
// ljmd_rhok.cpp, ljmd_current.cpp); g(r) and the pressure tensor dispatch a multi-device parent to its rank engines.
// MSD / VACF, the heat flux, the van Hove function, the density modes and the current modes take one-rank engines only:
// their cores refuse every other handle at configure, so a parent never has them configured.
#include "ljmd_engine.h"
#include "ljmd_multi.h"

namespace {

using ljmds::kStressWords;

ResidentView view_of(const ljmd_t *h)
{
    ResidentView v;
    v.n = h->n; v.S = h->plan.S; v.P = h->plan.P; v.TB = h->plan.TB; v.T = h->plan.T; v.G = h->G; v.rank = h->rank;
    v.multi = h->multi != nullptr;
    v.L = h->L; v.invL = h->invL; v.rc2 = h->rc2;
    v.pos = h->d_pos;
    v.ru = h->d_ru; v.v = h->d_v; v.perm = h->d_perm;
    v.stream = h->stream;
    v.compact = h->positions_compact;
    v.walk_chunk = h->knobs.walk_chunk;
    v.vanhove_chunk = h->knobs.vanhove_chunk;
    return v;
}

// one of the seven: whether it is configured on a handle, and the failure where it is not
struct Observable {
    bool (*configured)(const ljmd_t *h);
    int (*not_configured)(std::string *err, const char *who);
};
const Observable kRdf = {[](const ljmd_t *h) { return h->rdf.nbins != 0; }, ljmdr::not_configured};
const Observable kTcf = {[](const ljmd_t *h) { return h->tcf.max_lag != 0; }, ljmdt::not_configured};
const Observable kStress = {[](const ljmd_t *h) { return h->stress.max_snapshots != 0; }, ljmds::not_configured};
const Observable kHeatflux = {[](const ljmd_t *h) { return h->heatflux.max_snapshots != 0; }, ljmdq::not_configured};
const Observable kVanHove = {[](const ljmd_t *h) { return h->vanhove.max_lag != 0; }, ljmdv::not_configured};
const Observable kRhok = {[](const ljmd_t *h) { return h->rhok.max_snapshots != 0; }, ljmdc::not_configured};
const Observable kCurrent = {[](const ljmd_t *h) { return h->current.max_snapshots != 0; }, ljmdc::current_not_configured};

// a handle, and the observable configured on it
int configured(ljmd_t *h, const char *who, const Observable &o)
{
    LJMD_TRY(entry_checks(h, who, kHandle));
    return o.configured(h) ? LJMD_OK : o.not_configured(&h->err, who);
}

// the start of an accumulate; a multi-device parent leaves the last two to its ranks
int accumulate_checks(ljmd_t *h, const char *who, const Observable &o)
{
    LJMD_TRY(configured(h, who, o));
    LJMD_TRY(entry_checks(h, who, kHaveState | kHaveAccel | kNotPoisoned));
    if (h->multi) return LJMD_OK;
    // between ljmd_step_begin and ljmd_step_finish the own block is a step ahead of the other ranks' blocks
    if (h->step_open || h->forces_pending)
        return fail(h, LJMD_ERR_STATE, "%s: inside a split-phase step (call ljmd_step_finish first)", who);
    LJMD_HIP(h, hipSetDevice(h->device));
    return LJMD_OK;
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

// on(rank engine) configures a rank, off(rank engine) switches it off.  Every rank runs the same guards on the same
// arguments: a failed guard (LJMD_ERR_INVALID_ARG) stops at rank 0 with nothing changed
template <class On, class Off>
int configure_ranks(ljmd_t *h, On &&on, Off &&off)
{
    const int rc_ = for_ranks(h, on);
    if (rc_ == LJMD_ERR_INVALID_ARG) return rc_;
    if (rc_ != LJMD_OK) {                           // off everywhere; the first failure's message stays
        const std::string msg = h->err;
        (void)for_ranks(h, off);
        h->err = msg;
    }
    return rc_;
}

// ljmd_*_profile_read of a multi-device parent.  Tile pairs: sums over the ranks; time: the slowest rank
int profile_read_ranks(ljmd_t *h, int (*read)(ljmd_t *, int64_t *, int64_t *, double *), int64_t *tile_pairs_visited,
                       int64_t *tile_pairs_total, double *kernel_ms)
{
    int64_t vis = 0, tot = 0;
    double ms = 0.0;
    const int rc_ = for_ranks(h, [&](ljmd_t *e) {
        int64_t a = 0, b = 0;
        double t = 0.0;
        const int r = read(e, &a, &b, &t);
        vis += a; tot += b; ms = std::max(ms, t);
        return r;
    });
    if (rc_ != LJMD_OK) return rc_;
    if (tile_pairs_visited) *tile_pairs_visited = vis;
    if (tile_pairs_total) *tile_pairs_total = tot;
    if (kernel_ms) *kernel_ms = ms;
    return LJMD_OK;
}

// a multi-device parent: the sum of the ranks' partial words in 192 bits; the snapshot count is common to them
int stress_multi_fetch(ljmd_t *h, const char *who, std::vector<int64_t> *sum, int64_t *n_snapshots)
{
    if (!kStress.configured(h)) return kStress.not_configured(&h->err, who);
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

void ljmdh::release_resident(ljmd_t *h)
{
    ljmdr::rdf_release(&h->rdf, h->stream);
    ljmdt::tcf_release(&h->tcf, h->stream);
    ljmds::stress_release(&h->stress, h->stream);
    ljmdq::heatflux_release(&h->heatflux, h->stream);
    ljmdv::vanhove_release(&h->vanhove, h->stream);
    ljmdc::rhok_release(&h->rhok, h->stream);
    ljmdc::current_release(&h->current, h->stream);
}

extern "C" {

// ---- g(r) ------------------------------------------------------------------

int ljmd_rdf_configure(ljmd_t *h, int32_t nbins, double rmax)
{
    static const char *who = "ljmd_rdf_configure";
    static_assert(LJMD_RDF_MAX_BINS == ljmdr::kRdfMaxBins, "LJMD_RDF_MAX_BINS out of sync with the kernel");
    LJMD_TRY(entry_checks(h, who, kHandle));
    if (h->multi) {
        const int rc_ = configure_ranks(h, [&](ljmd_t *e) { return ljmd_rdf_configure(e, nbins, rmax); },
                                        [](ljmd_t *e) { return ljmd_rdf_configure(e, 0, 0.0); });
        if (rc_ == LJMD_ERR_INVALID_ARG) return rc_;
        h->rdf.nbins = rc_ == LJMD_OK ? nbins : 0;
        return rc_;
    }
    LJMD_HIP(h, hipSetDevice(h->device));
    return ljmdr::rdf_configure(&h->rdf, &h->err, who, view_of(h), nbins, rmax);
}

int ljmd_rdf_accumulate(ljmd_t *h)
{
    static const char *who = "ljmd_rdf_accumulate";
    LJMD_TRY(accumulate_checks(h, who, kRdf));
    if (h->multi) return for_ranks(h, [](ljmd_t *e) { return ljmd_rdf_accumulate(e); });
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
    LJMD_TRY(configured(h, who, kRdf));
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
        LJMD_TRY(configured(h, who, kRdf));
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
    LJMD_TRY(configured(h, who, kRdf));
    return profile_read_ranks(h, ljmd_rdf_profile_read, tile_pairs_visited, tile_pairs_total, kernel_ms);
}

// ---- MSD / VACF ------------------------------------------------------------

int ljmd_tcf_configure(ljmd_t *h, int32_t max_lag, int32_t origin_stride)
{
    static const char *who = "ljmd_tcf_configure";
    LJMD_TRY(entry_checks(h, who, kHandle));
    if (!h->multi) LJMD_HIP(h, hipSetDevice(h->device));
    return ljmdt::tcf_configure(&h->tcf, &h->err, who, view_of(h), max_lag, origin_stride);
}

int ljmd_tcf_accumulate(ljmd_t *h)
{
    static const char *who = "ljmd_tcf_accumulate";
    LJMD_TRY(accumulate_checks(h, who, kTcf));
    return ljmdt::tcf_accumulate(&h->tcf, &h->err, who, view_of(h));
}

int ljmd_tcf_read(ljmd_t *h, double *msd, double *vacf, int64_t *counts, int64_t *n_snapshots)
{
    static const char *who = "ljmd_tcf_read";
    LJMD_TRY(configured(h, who, kTcf));
    LJMD_HIP(h, hipSetDevice(h->device));
    return ljmdt::tcf_read(&h->tcf, &h->err, who, view_of(h), msd, vacf, counts, n_snapshots);
}

int ljmd_tcf_read_exact(ljmd_t *h, int64_t *words, int64_t *counts, int64_t *n_snapshots)
{
    static const char *who = "ljmd_tcf_read_exact";
    LJMD_TRY(configured(h, who, kTcf));
    LJMD_HIP(h, hipSetDevice(h->device));
    return ljmdt::tcf_fetch(&h->tcf, &h->err, who, view_of(h), reinterpret_cast<uint64_t *>(words), counts, n_snapshots);
}

int ljmd_tcf_reset(ljmd_t *h)
{
    static const char *who = "ljmd_tcf_reset";
    LJMD_TRY(configured(h, who, kTcf));
    LJMD_HIP(h, hipSetDevice(h->device));
    return ljmdt::tcf_reset(&h->tcf, &h->err, who, view_of(h));
}

int ljmd_tcf_profile_read(ljmd_t *h, double *kernel_ms, int32_t *origins_live)
{
    static const char *who = "ljmd_tcf_profile_read";
    LJMD_TRY(configured(h, who, kTcf));
    LJMD_HIP(h, hipSetDevice(h->device));
    return ljmdt::tcf_profile_read(&h->tcf, &h->err, who, view_of(h), kernel_ms, origins_live);
}

// ---- pressure tensor -------------------------------------------------------
// a multi-device parent counts the snapshots itself (its ranks count their own, all the same)

int ljmd_stress_configure(ljmd_t *h, int32_t max_snapshots)
{
    static const char *who = "ljmd_stress_configure";
    LJMD_TRY(entry_checks(h, who, kHandle));
    if (h->multi) {
        const int rc_ = configure_ranks(h, [&](ljmd_t *e) { return ljmd_stress_configure(e, max_snapshots); },
                                        [](ljmd_t *e) { return ljmd_stress_configure(e, 0); });
        if (rc_ == LJMD_ERR_INVALID_ARG) return rc_;
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
    LJMD_TRY(accumulate_checks(h, who, kStress));
    if (h->multi) {
        // a full series stops here, before any rank has launched anything
        if (h->stress.snapshots >= h->stress.max_snapshots)
            return fail(h, LJMD_ERR_STATE, "%s: the series is full (%d snapshots; read it, then ljmd_stress_reset)", who,
                        h->stress.max_snapshots);
        LJMD_TRY(for_ranks(h, [](ljmd_t *e) { return ljmd_stress_accumulate(e); }));
        ++h->stress.snapshots;
        return LJMD_OK;
    }
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
    LJMD_TRY(stress_multi_fetch(h, who, words ? &sum : nullptr, n_snapshots));
    if (words) std::copy(sum.begin(), sum.end(), words);
    return LJMD_OK;
}

int ljmd_stress_read(ljmd_t *h, double *p, int64_t *n_snapshots)
{
    static const char *who = "ljmd_stress_read";
    LJMD_TRY(entry_checks(h, who, kHandle));
    if (!h->multi) {
        LJMD_TRY(configured(h, who, kStress));
        if (h->G != 1)
            return fail(h, LJMD_ERR_STATE, "%s: a rank engine holds a partial sum (rank %d of %d): add the words of "
                                           "ljmd_stress_read_exact over the ranks and call ljmd_stress_from_exact", who, h->rank,
                        h->G);
        LJMD_HIP(h, hipSetDevice(h->device));
        return ljmds::stress_read(&h->stress, &h->err, who, view_of(h), p, n_snapshots);
    }
    std::vector<int64_t> sum;
    LJMD_TRY(stress_multi_fetch(h, who, p ? &sum : nullptr, n_snapshots));
    for (int64_t s = 0; p && s < h->stress.snapshots; ++s)
        ljmds::stress_doubles(sum.data() + (size_t)s * kStressWords, h->L, p + (size_t)s * ljmds::kStressComponents);
    return LJMD_OK;
}

int ljmd_stress_reset(ljmd_t *h)
{
    static const char *who = "ljmd_stress_reset";
    LJMD_TRY(entry_checks(h, who, kHandle));
    if (h->multi) {
        LJMD_TRY(configured(h, who, kStress));
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
    LJMD_TRY(configured(h, who, kStress));
    return profile_read_ranks(h, ljmd_stress_profile_read, tile_pairs_visited, tile_pairs_total, kernel_ms);
}

// ---- heat flux -------------------------------------------------------------
// one-rank engines only, as MSD / VACF: the core refuses every other handle at configure

int ljmd_heatflux_configure(ljmd_t *h, int32_t max_snapshots)
{
    static const char *who = "ljmd_heatflux_configure";
    LJMD_TRY(entry_checks(h, who, kHandle));
    if (!h->multi) LJMD_HIP(h, hipSetDevice(h->device));
    return ljmdq::heatflux_configure(&h->heatflux, &h->err, who, view_of(h), max_snapshots);
}

int ljmd_heatflux_accumulate(ljmd_t *h)
{
    static const char *who = "ljmd_heatflux_accumulate";
    LJMD_TRY(accumulate_checks(h, who, kHeatflux));
    return ljmdq::heatflux_accumulate(&h->heatflux, &h->err, who, view_of(h));
}

int ljmd_heatflux_read_exact(ljmd_t *h, int64_t *words, int64_t *n_snapshots)
{
    static const char *who = "ljmd_heatflux_read_exact";
    LJMD_TRY(configured(h, who, kHeatflux));
    LJMD_HIP(h, hipSetDevice(h->device));
    return ljmdq::heatflux_fetch(&h->heatflux, &h->err, who, view_of(h), words, n_snapshots);
}

int ljmd_heatflux_read(ljmd_t *h, double *j, double *parts, int64_t *n_snapshots)
{
    static const char *who = "ljmd_heatflux_read";
    LJMD_TRY(configured(h, who, kHeatflux));
    LJMD_HIP(h, hipSetDevice(h->device));
    return ljmdq::heatflux_read(&h->heatflux, &h->err, who, view_of(h), j, parts, n_snapshots);
}

int ljmd_heatflux_reset(ljmd_t *h)
{
    static const char *who = "ljmd_heatflux_reset";
    LJMD_TRY(configured(h, who, kHeatflux));
    LJMD_HIP(h, hipSetDevice(h->device));
    return ljmdq::heatflux_reset(&h->heatflux, &h->err, who, view_of(h));
}

int ljmd_heatflux_profile_read(ljmd_t *h, int64_t *tile_pairs_visited, int64_t *tile_pairs_total, double *kernel_ms)
{
    static const char *who = "ljmd_heatflux_profile_read";
    LJMD_TRY(configured(h, who, kHeatflux));
    LJMD_HIP(h, hipSetDevice(h->device));
    return ljmdq::heatflux_profile_read(&h->heatflux, &h->err, who, view_of(h), tile_pairs_visited, tile_pairs_total, kernel_ms);
}

// ---- van Hove self-correlation ---------------------------------------------
// one-rank engines only, as MSD / VACF: the core refuses every other handle at configure

int ljmd_vanhove_configure(ljmd_t *h, int32_t max_lag, int32_t origin_stride, int32_t nbins, double rmax)
{
    static const char *who = "ljmd_vanhove_configure";
    LJMD_TRY(entry_checks(h, who, kHandle));
    if (!h->multi) LJMD_HIP(h, hipSetDevice(h->device));
    return ljmdv::vanhove_configure(&h->vanhove, &h->err, who, view_of(h), max_lag, origin_stride, nbins, rmax);
}

int ljmd_vanhove_accumulate(ljmd_t *h)
{
    static const char *who = "ljmd_vanhove_accumulate";
    LJMD_TRY(accumulate_checks(h, who, kVanHove));
    return ljmdv::vanhove_accumulate(&h->vanhove, &h->err, who, view_of(h));
}

int ljmd_vanhove_read(ljmd_t *h, uint64_t *hist, double *r2, double *r4, int64_t *counts, int64_t *n_snapshots)
{
    static const char *who = "ljmd_vanhove_read";
    LJMD_TRY(configured(h, who, kVanHove));
    LJMD_HIP(h, hipSetDevice(h->device));
    return ljmdv::vanhove_read(&h->vanhove, &h->err, who, view_of(h), hist, r2, r4, counts, n_snapshots);
}

int ljmd_vanhove_read_exact(ljmd_t *h, uint64_t *hist, int64_t *words, int64_t *counts, int64_t *n_snapshots)
{
    static const char *who = "ljmd_vanhove_read_exact";
    LJMD_TRY(configured(h, who, kVanHove));
    LJMD_HIP(h, hipSetDevice(h->device));
    return ljmdv::vanhove_fetch(&h->vanhove, &h->err, who, view_of(h), hist, reinterpret_cast<uint64_t *>(words), counts,
                                n_snapshots);
}

int ljmd_vanhove_reset(ljmd_t *h)
{
    static const char *who = "ljmd_vanhove_reset";
    LJMD_TRY(configured(h, who, kVanHove));
    LJMD_HIP(h, hipSetDevice(h->device));
    return ljmdv::vanhove_reset(&h->vanhove, &h->err, who, view_of(h));
}

int ljmd_vanhove_profile_read(ljmd_t *h, double *kernel_ms, int32_t *origins_live)
{
    static const char *who = "ljmd_vanhove_profile_read";
    LJMD_TRY(configured(h, who, kVanHove));
    LJMD_HIP(h, hipSetDevice(h->device));
    return ljmdv::vanhove_profile_read(&h->vanhove, &h->err, who, view_of(h), kernel_ms, origins_live);
}

// ---- density modes ----------------------------------------------------------
// one-rank engines only, as MSD / VACF: the core refuses every other handle at configure

int ljmd_rhok_configure(ljmd_t *h, int32_t n_modes, const int32_t *modes, int32_t max_snapshots)
{
    static const char *who = "ljmd_rhok_configure";
    LJMD_TRY(entry_checks(h, who, kHandle));
    if (!h->multi) LJMD_HIP(h, hipSetDevice(h->device));
    return ljmdc::rhok_configure(&h->rhok, &h->err, who, view_of(h), n_modes, modes, max_snapshots);
}

int ljmd_rhok_accumulate(ljmd_t *h)
{
    static const char *who = "ljmd_rhok_accumulate";
    LJMD_TRY(configured(h, who, kRhok));
    // the positions alone: a state, but no accelerations
    LJMD_TRY(entry_checks(h, who, kHaveState | kNotPoisoned));
    if (h->step_open || h->forces_pending)
        return fail(h, LJMD_ERR_STATE, "%s: inside a split-phase step (call ljmd_step_finish first)", who);
    LJMD_HIP(h, hipSetDevice(h->device));
    return ljmdc::rhok_accumulate(&h->rhok, &h->err, who, view_of(h));
}

int ljmd_rhok_read_exact(ljmd_t *h, int64_t *words, int64_t *n_snapshots)
{
    static const char *who = "ljmd_rhok_read_exact";
    LJMD_TRY(configured(h, who, kRhok));
    LJMD_HIP(h, hipSetDevice(h->device));
    return ljmdc::rhok_fetch(&h->rhok, &h->err, who, view_of(h), words, n_snapshots);
}

int ljmd_rhok_read(ljmd_t *h, double *rho, int64_t *n_snapshots)
{
    static const char *who = "ljmd_rhok_read";
    LJMD_TRY(configured(h, who, kRhok));
    LJMD_HIP(h, hipSetDevice(h->device));
    return ljmdc::rhok_read(&h->rhok, &h->err, who, view_of(h), rho, n_snapshots);
}

int ljmd_rhok_reset(ljmd_t *h)
{
    static const char *who = "ljmd_rhok_reset";
    LJMD_TRY(configured(h, who, kRhok));
    LJMD_HIP(h, hipSetDevice(h->device));
    return ljmdc::rhok_reset(&h->rhok, &h->err, who, view_of(h));
}

int ljmd_rhok_profile_read(ljmd_t *h, double *kernel_ms)
{
    static const char *who = "ljmd_rhok_profile_read";
    LJMD_TRY(configured(h, who, kRhok));
    LJMD_HIP(h, hipSetDevice(h->device));
    return ljmdc::rhok_profile_read(&h->rhok, &h->err, who, view_of(h), kernel_ms);
}

// ---- current modes ----------------------------------------------------------
// one-rank engines only, as MSD / VACF: the core refuses every other handle at configure

int ljmd_current_configure(ljmd_t *h, int32_t n_modes, const int32_t *modes, int32_t max_snapshots)
{
    static const char *who = "ljmd_current_configure";
    LJMD_TRY(entry_checks(h, who, kHandle));
    if (!h->multi) LJMD_HIP(h, hipSetDevice(h->device));
    return ljmdc::current_configure(&h->current, &h->err, who, view_of(h), n_modes, modes, max_snapshots);
}

int ljmd_current_accumulate(ljmd_t *h)
{
    static const char *who = "ljmd_current_accumulate";
    LJMD_TRY(configured(h, who, kCurrent));
    // the positions and velocities alone: a state, but no accelerations
    LJMD_TRY(entry_checks(h, who, kHaveState | kNotPoisoned));
    if (h->step_open || h->forces_pending)
        return fail(h, LJMD_ERR_STATE, "%s: inside a split-phase step (call ljmd_step_finish first)", who);
    LJMD_HIP(h, hipSetDevice(h->device));
    return ljmdc::current_accumulate(&h->current, &h->err, who, view_of(h));
}

int ljmd_current_read_exact(ljmd_t *h, int64_t *words, int64_t *n_snapshots)
{
    static const char *who = "ljmd_current_read_exact";
    LJMD_TRY(configured(h, who, kCurrent));
    LJMD_HIP(h, hipSetDevice(h->device));
    return ljmdc::current_fetch(&h->current, &h->err, who, view_of(h), words, n_snapshots);
}

int ljmd_current_read(ljmd_t *h, double *j, int64_t *n_snapshots)
{
    static const char *who = "ljmd_current_read";
    LJMD_TRY(configured(h, who, kCurrent));
    LJMD_HIP(h, hipSetDevice(h->device));
    return ljmdc::current_read(&h->current, &h->err, who, view_of(h), j, n_snapshots);
}

int ljmd_current_reset(ljmd_t *h)
{
    static const char *who = "ljmd_current_reset";
    LJMD_TRY(configured(h, who, kCurrent));
    LJMD_HIP(h, hipSetDevice(h->device));
    return ljmdc::current_reset(&h->current, &h->err, who, view_of(h));
}

int ljmd_current_profile_read(ljmd_t *h, double *kernel_ms)
{
    static const char *who = "ljmd_current_profile_read";
    LJMD_TRY(configured(h, who, kCurrent));
    LJMD_HIP(h, hipSetDevice(h->device));
    return ljmdc::current_profile_read(&h->current, &h->err, who, view_of(h), kernel_ms);
}

}  // extern "C"
