// ljmd_heatflux.cpp -- the engine's resident heat flux on the host (kernels: ljmd_heatflux.hip): its descriptor for the
// series core (ljmd_series.cpp), the arguments of its pair kernel, the conversion to doubles, and
// ljmd_heatflux_from_exact, which needs no engine.  Like the core it sees an engine only through ResidentView and links
// without anything of struct ljmd (tests/heatflux_host); the C entry points that take a handle are in ljmd_resident.cpp.
#include "ljmd_resident.h"

#include <cmath>

using namespace ljmdh;

namespace ljmdq {

namespace {

hipError_t launch(const HeatfluxState &st, const ResidentView &v, const ljmdr::RdfWalk &w, const HeatfluxKineticArgs &ka,
                  const HeatfluxFoldArgs &fa)
{
    HeatfluxPairArgs pa{};
    pa.pos = v.pos;
    pa.vel = v.v;
    pa.bbox = st.d_bbox;
    pa.part = st.d_part; pa.pcount = st.d_pcount; pa.pflag = st.d_pflag;
    pa.P = v.P; pa.T = v.T;
    pa.U = w.U; pa.chunk = w.chunk;
    pa.skip = v.compact ? 1 : 0;
    pa.L = v.L; pa.invL = v.invL; pa.rc2 = v.rc2;
    pa.rc2_skin = v.rc2 * (1.0 + 1e-10);
    hipError_t e = launch_heatflux_pairs(pa, dim3(w.row_blocks, w.slices), v.stream);
    if (e == hipSuccess) e = launch_heatflux_kinetic(ka, v.stream);
    if (e == hipSuccess) e = launch_heatflux_fold(fa, v.stream);
    return e;
}

static_assert(kHeatfluxMaxSnapshots == LJMD_HEATFLUX_MAX_SNAPSHOTS, "LJMD_HEATFLUX_MAX_SNAPSHOTS out of sync with the core");
static_assert(kHeatfluxMaxN == ljmdk::kFixedMaxN, "the lane accumulators rest on kFixedMaxN");

// one-rank engines only: configure refuses a multi-device handle and a rank engine of G > 1
const SeriesDesc kDesc = {"heat flux", "heatflux", "the convective partials", "the convective flags", kHeatfluxWords,
                          kHeatfluxPairComponents, kHeatfluxKinComponents, kHeatfluxMaxSnapshots, kHeatfluxMaxN,
                          kHeatfluxKinBlock, true, launch};

}  // namespace

int not_configured(std::string *err, const char *who) { return series_not_configured(kDesc, err, who); }
void heatflux_release(HeatfluxState *st, hipStream_t stream) { series_release(kDesc, st, stream); }

int heatflux_configure(HeatfluxState *st, std::string *err, const char *who, const ResidentView &v, int32_t max_snapshots)
{
    return series_configure(kDesc, st, err, who, v, max_snapshots);
}

int heatflux_accumulate(HeatfluxState *st, std::string *err, const char *who, const ResidentView &v)
{
    return series_accumulate(kDesc, st, err, who, v);
}

int heatflux_fetch(HeatfluxState *st, std::string *err, const char *who, const ResidentView &v, int64_t *words, int64_t *n_snapshots)
{
    return series_fetch(kDesc, st, err, who, v, words, n_snapshots);
}

int heatflux_read(HeatfluxState *st, std::string *err, const char *who, const ResidentView &v, double *j, double *parts,
                  int64_t *n_snapshots)
{
    const bool want = j || parts;
    std::vector<int64_t> w;
    LJMD_TRY(series_read_words(kDesc, st, err, who, v, want, &w, n_snapshots));
    for (int64_t s = 0; want && s < st->snapshots; ++s)
        heatflux_doubles(w.data() + (size_t)s * kHeatfluxWords, v.L, j ? j + (size_t)s * 3 : nullptr,
                         parts ? parts + (size_t)s * 9 : nullptr);
    return LJMD_OK;
}

int heatflux_reset(HeatfluxState *st, std::string *err, const char *who, const ResidentView &v)
{
    return series_reset(kDesc, st, err, who, v);
}

int heatflux_profile_read(HeatfluxState *st, std::string *err, const char *who, const ResidentView &v, int64_t *visited,
                          int64_t *total, double *kernel_ms)
{
    return series_profile_read(kDesc, st, err, who, v, visited, total, kernel_ms);
}

}  // namespace ljmdq

extern "C" int ljmd_heatflux_from_exact(const int64_t *words, double box_length, double *j3, double *parts9)
{
    if (!words || !j3) return fail(nullptr, LJMD_ERR_INVALID_ARG, "ljmd_heatflux_from_exact: NULL argument");
    if (!(std::isfinite(box_length) && box_length > 0.0))
        return fail(nullptr, LJMD_ERR_INVALID_ARG, "ljmd_heatflux_from_exact: box_length must be finite and > 0");
    ljmdq::heatflux_doubles(words, box_length, j3, parts9);
    return LJMD_OK;
}
