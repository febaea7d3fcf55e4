// ljmd_profile.cpp -- measurement entry points of the C ABI: which pair kernel runs, and the read-out of the per-launch
// event sets (ljmd_engine.h: EventSet).
#include "ljmd_engine.h"
#include "ljmd_multi.h"

extern "C" {

const char *ljmd_pair_kernel_name(const ljmd_t *h)
{
    if (!h) return "";
    if (h->multi) return ljmdm::pair_kernel_name(h);
    if (reproducible(h)) return "pair_fixed_kernel";
    if (!fast_path_ok(h)) return "pair_rows_generic_kernel";
    if (h->plan.use_n3 && h->mode == LJMD_PRECISION_FP32_FORCE) return "pair_n3_f32_kernel";
    return h->plan.use_n3 ? "pair_n3_kernel" : "pair_tiles_kernel";
}

int ljmd_profile_enable(ljmd_t *h, int32_t on)
{
    LJMD_TRY(entry_checks(h, "ljmd_profile_enable", kHandle));
    if (h->multi) return ljmdm::profile_enable(h, on);
    h->profiling = on != 0;
    h->ev_used = 0;
    return LJMD_OK;
}

int ljmd_profile_read(ljmd_t *h, double *ms_avg, int32_t *launches)
{
    return ljmd_profile_read_ex(h, ms_avg, nullptr, launches);
}

namespace {
// intervals 0..3 as documented for ljmd_profile_read; 4 = position exchange, 5 = force exchange (averages over the
// launches that had one; 0 when none did)
int profile_read_full(ljmd_t *h, double *ms_avg /* [6] */, double *ms_min /* [6] */, int32_t *launches,
                      double *ms_median = nullptr /* [6] */)
{
    LJMD_HIP(h, hipSetDevice(h->device));
    LJMD_HIP(h, hipStreamSynchronize(h->stream));
    if (h->comm_stream) LJMD_HIP(h, hipStreamSynchronize(h->comm_stream));
    double acc[6] = {0, 0, 0, 0, 0, 0};  // pair kernel, geometry pre-pass, drift/kick, reduce+finalize, exchanges
    double lo[6] = {1e300, 1e300, 1e300, 1e300, 1e300, 1e300};
    size_t cnt_x[2] = {0, 0};
    std::vector<double> all[6];              // per launch, for the medians
    const int from[6] = {2, 1, 0, 3, 5, 7}, to[6] = {3, 2, 1, 4, 6, 8};
    size_t complete = 0;
    for (size_t k = 0; k < h->ev_used; ++k) {
        const EventSet &q = h->ev_pool[k];
        double one[6] = {0, 0, 0, 0, 0, 0};
        bool ok = true;
        for (int c = 0; c < 4 && ok; ++c) {
            float ms = 0.f;   // a set whose step was only half enqueued has unrecorded events: skip it
            ok = hipEventElapsedTime(&ms, q.e[from[c]], q.e[to[c]]) == hipSuccess;
            one[c] = ms;
        }
        if (!ok) {
            (void)hipGetLastError();
            continue;
        }
        const bool have[2] = {q.has_pos_x, q.has_force_x};
        for (int x = 0; x < 2; ++x) {
            float ms = 0.f;
            if (have[x] && hipEventElapsedTime(&ms, q.e[from[4 + x]], q.e[to[4 + x]]) == hipSuccess) {
                acc[4 + x] += ms;
                lo[4 + x] = std::min(lo[4 + x], (double)ms);
                all[4 + x].push_back(ms);
                ++cnt_x[x];
            } else if (have[x]) {
                (void)hipGetLastError();
            }
        }
        for (int c = 0; c < 4; ++c) {
            acc[c] += one[c];
            lo[c] = std::min(lo[c], one[c]);
            all[c].push_back(one[c]);
        }
        ++complete;
    }
    h->ev_used = complete;
    const double cnt = h->ev_used ? (double)h->ev_used : 1.0;
    for (int c = 0; c < 6; ++c) {
        const double div = c < 4 ? cnt : (cnt_x[c - 4] ? (double)cnt_x[c - 4] : 1.0);
        const bool any = c < 4 ? h->ev_used > 0 : cnt_x[c - 4] > 0;
        if (ms_avg) ms_avg[c] = acc[c] / div;
        if (ms_min) ms_min[c] = any ? lo[c] : 0.0;
        if (ms_median) {
            std::vector<double> &v = all[c];
            std::sort(v.begin(), v.end());
            const size_t m = v.size();
            ms_median[c] = m == 0 ? 0.0 : (m % 2 ? v[m / 2] : 0.5 * (v[m / 2 - 1] + v[m / 2]));
        }
    }
    if (launches) *launches = (int32_t)h->ev_used;
    h->ev_used = 0;
    return LJMD_OK;
}
}  // namespace

int ljmd_profile_read_ex(ljmd_t *h, double *ms_avg, double *ms_min, int32_t *launches)
{
    LJMD_TRY(entry_checks(h, "ljmd_profile_read", kHandle));
    if (h->multi) return ljmdm::profile_read_ex(h, ms_avg, ms_min, launches);
    double a[6], b[6];
    const int rc_ = profile_read_full(h, a, b, launches);
    if (rc_ != LJMD_OK) return rc_;
    if (ms_avg) std::memcpy(ms_avg, a, 4 * sizeof(double));
    if (ms_min) std::memcpy(ms_min, b, 4 * sizeof(double));
    return LJMD_OK;
}

int ljmd_profile_read_rank(ljmd_t *h, int32_t rank, double *ms_avg, double *ms_min, int32_t *launches)
{
    LJMD_TRY(entry_checks(h, "ljmd_profile_read_rank", kHandle));
    if (h->multi) {
        ljmd_t *e = ljmdm::rank_engine(h, rank);
        if (!e) return fail(h, LJMD_ERR_INVALID_ARG, "ljmd_profile_read_rank: rank %d out of range", rank);
        const int rc_ = profile_read_full(e, ms_avg, ms_min, launches);
        if (rc_ != LJMD_OK) return fail(h, rc_, "rank %d (device %d): %s", e->rank, e->device, e->err.c_str());
        return LJMD_OK;
    }
    if (rank != h->rank) return fail(h, LJMD_ERR_INVALID_ARG, "ljmd_profile_read_rank: this engine is rank %d", h->rank);
    return profile_read_full(h, ms_avg, ms_min, launches);
}

int ljmd_profile_read_stats(ljmd_t *h, int32_t rank, double *ms_avg, double *ms_min, double *ms_median, int32_t *launches)
{
    LJMD_TRY(entry_checks(h, "ljmd_profile_read_stats", kHandle));
    if (h->multi) {
        ljmd_t *e = ljmdm::rank_engine(h, rank);
        if (!e) return fail(h, LJMD_ERR_INVALID_ARG, "ljmd_profile_read_stats: rank %d out of range", rank);
        const int rc_ = profile_read_full(e, ms_avg, ms_min, launches, ms_median);
        if (rc_ != LJMD_OK) return fail(h, rc_, "rank %d (device %d): %s", e->rank, e->device, e->err.c_str());
        return LJMD_OK;
    }
    if (rank != h->rank) return fail(h, LJMD_ERR_INVALID_ARG, "ljmd_profile_read_stats: this engine is rank %d", h->rank);
    return profile_read_full(h, ms_avg, ms_min, launches, ms_median);
}

}  // extern "C"
