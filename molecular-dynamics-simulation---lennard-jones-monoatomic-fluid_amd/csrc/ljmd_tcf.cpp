// ljmd_tcf.cpp -- the engine's resident MSD / VACF on the host (kernels: ljmd_tcf.hip): its descriptor for the time-origin
// core (ljmd_origins.cpp) and the arguments of its terms kernel.  Like the core it sees an engine only through
// ResidentView and links without anything of struct ljmd (tests/tcf_host); the C entry points are in ljmd_resident.cpp.
#include "ljmd_resident.h"

using namespace ljmdh;

namespace ljmdt {

namespace {

hipError_t launch(const TcfState &st, const ResidentView &v, const TcfWindow &w, const TcfSlices &p, const TcfGatherArgs &ga,
                  const TcfFoldArgs &fa)
{
    hipError_t e = launch_tcf_gather(ga, v.stream);
    if (e != hipSuccess || w.n_live == 0) return e;
    TcfTermsArgs ta{};
    ta.cur = st.d_cur; ta.ring = st.d_ring; ta.part = st.d_part; ta.flag = st.d_flag;
    ta.n_pad = st.sz.n_pad;
    ta.nblk = st.sz.nblk; ta.slots = st.sz.slots; ta.ents = st.sz.ents; ta.stride = st.stride;
    ta.n_live = w.n_live; ta.lag_first = w.lag_first; ta.slot_first = w.slot_first;
    ta.chunk = p.chunk; ta.slices = p.slices;
    e = launch_tcf_terms(ta, v.stream);
    return e != hipSuccess ? e : launch_tcf_fold(fa, v.stream);
}

static_assert(kTcfMaxLag == LJMD_TCF_MAX_LAG && kTcfMaxOrigins == LJMD_TCF_MAX_ORIGINS,
              "MSD / VACF limits out of sync with include/ljmd.h");

const OriginDesc kDesc = {"MSD / VACF", "MSD / VACF", "tcf", "TCF",
                          "an MSD or VACF term was not finite or |term| >= 2^40 and entered as 0",
                          6, true, kTcfMaxLag, kTcfMaxOrigins, kTcfMaxN, 0, false, launch};

}  // namespace

int not_configured(std::string *err, const char *who) { return origin_not_configured(kDesc, err, who); }
TcfSizes tcf_sizes(int n, int max_lag, int stride) { return origin_sizes(kDesc, n, max_lag, stride, 0); }
TcfSlices tcf_plan_slices(int nblk, int n_live) { return origin_plan_slices(nblk, n_live); }
void tcf_release(TcfState *st, hipStream_t stream) { origin_release(st, stream); }
void tcf_new_trajectory(TcfState *st) { origin_new_trajectory(st); }

int tcf_configure(TcfState *st, std::string *err, const char *who, const ResidentView &v, int32_t max_lag, int32_t origin_stride)
{
    return origin_configure(kDesc, st, err, who, v, max_lag, origin_stride, 0, 0.0);
}

int tcf_accumulate(TcfState *st, std::string *err, const char *who, const ResidentView &v)
{
    return origin_accumulate(kDesc, st, err, who, v);
}

int tcf_fetch(TcfState *st, std::string *err, const char *who, const ResidentView &v, uint64_t *words, int64_t *counts,
              int64_t *n_snapshots)
{
    return origin_fetch(kDesc, st, err, who, v, nullptr, words, counts, n_snapshots);
}

int tcf_read(TcfState *st, std::string *err, const char *who, const ResidentView &v, double *msd, double *vacf, int64_t *counts,
             int64_t *n_snapshots)
{
    return origin_read(kDesc, st, err, who, v, nullptr, msd, vacf, counts, n_snapshots);
}

int tcf_reset(TcfState *st, std::string *err, const char *who, const ResidentView &v)
{
    return origin_reset(kDesc, st, err, who, v);
}

int tcf_profile_read(TcfState *st, std::string *err, const char *who, const ResidentView &v, double *kernel_ms,
                     int32_t *origins_live)
{
    return origin_profile_read(kDesc, st, err, who, v, kernel_ms, origins_live);
}

}  // namespace ljmdt
