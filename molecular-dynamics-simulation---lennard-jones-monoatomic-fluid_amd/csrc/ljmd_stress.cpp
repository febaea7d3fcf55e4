// ljmd_stress.cpp -- the engine's resident pressure tensor on the host (kernels: ljmd_stress.hip): its descriptor for the
// series core (ljmd_series.cpp), the arguments of its pair kernel, the conversion to doubles, and ljmd_stress_from_exact,
// which needs no engine.  Like the core it sees an engine only through ResidentView and links without anything of struct
// ljmd (tests/stress_host); the C entry points that take a handle are in ljmd_resident.cpp.
#include "ljmd_resident.h"

#include <cmath>

using namespace ljmdh;

namespace ljmds {

namespace {

hipError_t launch(const StressState &st, const ResidentView &v, const ljmdr::RdfWalk &w, const StressKineticArgs &ka,
                  const StressFoldArgs &fa)
{
    StressPairArgs pa{};
    pa.pos = v.pos;
    pa.bbox = st.d_bbox;
    pa.part = st.d_part; pa.pcount = st.d_pcount; pa.pflag = st.d_pflag;
    pa.P = v.P; pa.G = v.G; pa.rank = v.rank; pa.TB = v.TB; pa.T = v.T;
    pa.U = w.U; pa.chunk = w.chunk;
    pa.skip = v.compact ? 1 : 0;
    pa.L = v.L; pa.invL = v.invL; pa.rc2 = v.rc2;
    pa.rc2_skin = v.rc2 * (1.0 + 1e-10);
    hipError_t e = launch_stress_pairs(pa, dim3(w.row_blocks, w.slices), v.stream);
    if (e == hipSuccess) e = launch_stress_kinetic(ka, v.stream);
    if (e == hipSuccess) e = launch_stress_fold(fa, v.stream);
    return e;
}

static_assert(kStressMaxSnapshots == LJMD_STRESS_MAX_SNAPSHOTS, "LJMD_STRESS_MAX_SNAPSHOTS out of sync with the core");
static_assert(kStressMaxN == ljmdk::kFixedMaxN, "the lane accumulators rest on kFixedMaxN");

const SeriesDesc kDesc = {"pressure tensor", "stress", "the kinetic partials", "the kinetic flags", kStressWords,
                          kStressComponents, kStressComponents, kStressMaxSnapshots, kStressMaxN, kStressKinBlock,
                          false, launch};

}  // namespace

int not_configured(std::string *err, const char *who) { return series_not_configured(kDesc, err, who); }
void stress_release(StressState *st, hipStream_t stream) { series_release(kDesc, st, stream); }

int stress_configure(StressState *st, std::string *err, const char *who, const ResidentView &v, int32_t max_snapshots)
{
    return series_configure(kDesc, st, err, who, v, max_snapshots);
}

int stress_accumulate(StressState *st, std::string *err, const char *who, const ResidentView &v)
{
    return series_accumulate(kDesc, st, err, who, v);
}

int stress_fetch(StressState *st, std::string *err, const char *who, const ResidentView &v, int64_t *words, int64_t *n_snapshots)
{
    return series_fetch(kDesc, st, err, who, v, words, n_snapshots);
}

int stress_read(StressState *st, std::string *err, const char *who, const ResidentView &v, double *p, int64_t *n_snapshots)
{
    std::vector<int64_t> w;
    LJMD_TRY(series_read_words(kDesc, st, err, who, v, p != nullptr, &w, n_snapshots));
    for (int64_t s = 0; p && s < st->snapshots; ++s)
        stress_doubles(w.data() + (size_t)s * kStressWords, v.L, p + (size_t)s * kStressComponents);
    return LJMD_OK;
}

int stress_reset(StressState *st, std::string *err, const char *who, const ResidentView &v)
{
    return series_reset(kDesc, st, err, who, v);
}

int stress_profile_read(StressState *st, std::string *err, const char *who, const ResidentView &v, int64_t *visited,
                        int64_t *total, double *kernel_ms)
{
    return series_profile_read(kDesc, st, err, who, v, visited, total, kernel_ms);
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
