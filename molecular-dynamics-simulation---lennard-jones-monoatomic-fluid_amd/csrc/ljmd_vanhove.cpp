// ljmd_vanhove.cpp -- the engine's resident van Hove self-correlation on the host (kernels: ljmd_vanhove.hip): its
// descriptor for the time-origin core (ljmd_origins.cpp) and the arguments of its terms kernel.  Like the core it sees an
// engine only through ResidentView and links without anything of struct ljmd (tests/vanhove_host); the C entry points
// are in ljmd_resident.cpp.
#include "ljmd_resident.h"

using namespace ljmdh;

namespace ljmdv {

namespace {

hipError_t launch(const VanHoveState &st, const ResidentView &v, const TcfWindow &w, const VhSlices &p, const VhGatherArgs &ga,
                  const VhFoldArgs &fa)
{
    hipError_t e = launch_vanhove_gather(ga, v.stream);
    if (e != hipSuccess || w.n_live == 0) return e;
    VhTermsArgs ta{};
    ta.cur = st.d_cur; ta.ring = st.d_ring; ta.hist = st.d_hist; ta.part = st.d_part; ta.flag = st.d_flag;
    ta.n_pad = st.sz.n_pad;
    ta.dr = st.dr; ta.inv_dr = st.inv_dr;
    ta.n = st.n; ta.nbins = st.nbins; ta.max_lag = st.max_lag;
    ta.nblk = st.sz.nblk; ta.slots = st.sz.slots; ta.ents = st.sz.ents; ta.stride = st.stride;
    ta.n_live = w.n_live; ta.lag_first = w.lag_first; ta.slot_first = w.slot_first;
    ta.chunk = p.chunk; ta.slices = p.slices;
    e = launch_vanhove_terms(ta, v.stream);
    return e != hipSuccess ? e : launch_vanhove_fold(fa, v.stream);
}

static_assert(kVhMaxLag == LJMD_VANHOVE_MAX_LAG && kVhMaxOrigins == LJMD_VANHOVE_MAX_ORIGINS &&
                  kVhMaxBins == LJMD_VANHOVE_MAX_BINS, "van Hove limits out of sync with include/ljmd.h");

const OriginDesc kDesc = {"the van Hove function", "van Hove", "vanhove", "VANHOVE",
                          "a van Hove displacement was not finite or r^4 >= 2^40: it was counted in the overflow column and "
                          "entered the sums as 0",
                          3, false, kVhMaxLag, kVhMaxOrigins, kVhMaxN, kVhMaxBins, true, launch};

}  // namespace

int not_configured(std::string *err, const char *who) { return origin_not_configured(kDesc, err, who); }
VhSizes vanhove_sizes(int n, int max_lag, int stride, int nbins) { return origin_sizes(kDesc, n, max_lag, stride, nbins); }
VhSlices vanhove_plan_slices(int nblk, int n_live, std::optional<int> chunk) { return origin_plan_slices(nblk, n_live, chunk); }
void vanhove_release(VanHoveState *st, hipStream_t stream) { origin_release(st, stream); }
void vanhove_new_trajectory(VanHoveState *st) { origin_new_trajectory(st); }

int vanhove_configure(VanHoveState *st, std::string *err, const char *who, const ResidentView &v, int32_t max_lag,
                      int32_t origin_stride, int32_t nbins, double rmax)
{
    return origin_configure(kDesc, st, err, who, v, max_lag, origin_stride, nbins, rmax);
}

int vanhove_accumulate(VanHoveState *st, std::string *err, const char *who, const ResidentView &v)
{
    return origin_accumulate(kDesc, st, err, who, v);
}

int vanhove_fetch(VanHoveState *st, std::string *err, const char *who, const ResidentView &v, uint64_t *hist, uint64_t *words,
                  int64_t *counts, int64_t *n_snapshots)
{
    return origin_fetch(kDesc, st, err, who, v, hist, words, counts, n_snapshots);
}

int vanhove_read(VanHoveState *st, std::string *err, const char *who, const ResidentView &v, uint64_t *hist, double *r2,
                 double *r4, int64_t *counts, int64_t *n_snapshots)
{
    return origin_read(kDesc, st, err, who, v, hist, r2, r4, counts, n_snapshots);
}

int vanhove_reset(VanHoveState *st, std::string *err, const char *who, const ResidentView &v)
{
    return origin_reset(kDesc, st, err, who, v);
}

int vanhove_profile_read(VanHoveState *st, std::string *err, const char *who, const ResidentView &v, double *kernel_ms,
                         int32_t *origins_live)
{
    return origin_profile_read(kDesc, st, err, who, v, kernel_ms, origins_live);
}

}  // namespace ljmdv
