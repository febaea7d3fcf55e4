// ljmd_common.cpp -- error reporting, parameter guards, derived parameters, the device probe, the table of environment
// knobs and the formulas from summed pair terms to the four scalars: shared by the single, multi-device and batch engine.
#include "ljmd_common.h"
#include "ljmd_internal.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <limits>

namespace ljmdh {

using namespace ljmdk;        // add192, fixed_to_double

thread_local std::string g_last_error = "";

int failv(std::string *handle_err, int code, const char *fmt, va_list ap)
{
    char buf[512];
    vsnprintf(buf, sizeof buf, fmt, ap);
    g_last_error = buf;
    if (handle_err) *handle_err = buf;
    return code;
}

int check_sim_params(const char *who, int n, double box_length, double dt, double rc)
{
    if (n <= 0) return fail(nullptr, LJMD_ERR_INVALID_ARG, "%s: n must be > 0", who);
    if (!(box_length > 0.0)) return fail(nullptr, LJMD_ERR_INVALID_ARG, "%s: box_length must be > 0", who);
    if (!(rc > 0.0)) return fail(nullptr, LJMD_ERR_INVALID_ARG, "%s: rc must be > 0", who);
    if (rc >= 0.5 * box_length)
        return fail(nullptr, LJMD_ERR_INVALID_ARG, "%s: rc must be < L/2 (minimum image convention)", who);
    if (!(dt > 0.0)) return fail(nullptr, LJMD_ERR_INVALID_ARG, "%s: dt must be > 0", who);
    return LJMD_OK;
}

int probe_device(int device, const char *who)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(nullptr, LJMD_ERR_NO_DEVICE, "%s: no HIP device available (this library has no CPU path)", who);
    if (device < 0 || device >= ndev)
        return fail(nullptr, LJMD_ERR_INVALID_ARG, "%s: device %d out of range (0..%d)", who, device, ndev - 1);
    return LJMD_OK;
}

// compute_derived_params, md_types.f90:137-159, same expressions
SimParams derive_params(int n, double box_length, double dt, double rc)
{
    SimParams p;
    p.L = box_length;
    p.invL = 1.0 / box_length;
    p.volume = box_length * box_length * box_length;
    p.rc = rc;
    p.rc2 = rc * rc;
    p.dt = dt;
    p.dt_half = 0.5 * dt;
    p.dt_sq_half = p.dt_half * dt;
    {   // tail corrections, lj_potential_energy.f90:205-223
        const double npd = (double)n;
        const double rc3 = (rc * rc) * rc;
        const double rc6 = ((rc * rc) * (rc * rc)) * (rc * rc);
        const double tf = 8.0 * kPi * (npd * npd) / (p.volume * rc3);
        p.tail_e = tf * ((1.0 / (3.0 * rc6)) - 1.0) / 3.0;
        p.tail_d = 2.0 * tf * (-2.0 / (3.0 * rc6) + 1.0);
        p.tail_dd = 2.0 * tf * (26.0 / (3.0 * rc6) - 7.0);
    }
    return p;
}

Knobs read_knobs()
{
    auto flag = [](const char *name, bool dflt) { return env_int(name, dflt ? 1 : 0) != 0; };
    auto is = [](const char *name, const char *value) {
        const char *v = std::getenv(name);
        return v && std::strcmp(v, value) == 0;
    };
    auto opt_int = [](const char *name) -> std::optional<int> {
        const char *v = std::getenv(name);
        if (v && *v) return std::atoi(v);
        return std::nullopt;
    };
    Knobs k;
    k.sort = flag("LJMD_SORT", k.sort);
    k.force_generic = flag("LJMD_FORCE_GENERIC", k.force_generic);
    k.force_collectives = flag("LJMD_FORCE_COLLECTIVES", k.force_collectives);
    k.fuse = flag("LJMD_FUSE", k.fuse);
    k.fuse_tail = flag("LJMD_FUSE_TAIL", k.fuse_tail);
    k.fuse_defer_record = flag("LJMD_FUSE_DEFER_RECORD", k.fuse_defer_record);
    // measured at n = 262144: chunks of 4 consecutive row groups per XCD -3 % pair-kernel time (19.8 -> 19.1 ms; 2: -1 %,
    // 8 / 16 / 32: +-0, one contiguous eighth per XCD: +10 %), -1.5 % at n = 131072 and 524288 (profiles/r02_xcd_remap_and_prefetch.txt)
    k.xcd_remap = std::max(0, env_int("LJMD_N3_XCD_REMAP", k.xcd_remap));
    k.inject_failure_at_step = env_int("LJMD_INJECT_FAILURE_AT_STEP", k.inject_failure_at_step);
    k.exchange_alltoall = is("LJMD_FORCE_EXCHANGE", "alltoall");
    k.resort_every = opt_int("LJMD_RESORT_EVERY");
    k.kd_sort_cub = is("LJMD_KD_SORT", "cub");
    k.n3_row_tiles = env_int("LJMD_N3_ROW_TILES", k.n3_row_tiles);
    k.n3_wg_waves = env_int("LJMD_N3_WG_WAVES", k.n3_wg_waves);
    k.slab_budget_gb = std::max(1, env_int("LJMD_SLAB_BUDGET_GB", k.slab_budget_gb));
    k.n3_both_ties = flag("LJMD_N3_BOTH_TIES", k.n3_both_ties);
    k.n3_min_n = env_int("LJMD_N3_MIN_N", k.n3_min_n);
    k.n3 = flag("LJMD_N3", k.n3);
    k.n3_target_waves = opt_int("LJMD_N3_TARGET_WAVES");
    k.n3_clusters = flag("LJMD_N3_CLUSTERS", k.n3_clusters);
    k.n3_pertile = flag("LJMD_N3_PERTILE", k.n3_pertile);
    k.reduce_split = opt_int("LJMD_REDUCE_SPLIT");
    if (k.reduce_split) k.reduce_split = std::max(0, *k.reduce_split);
    k.walk_chunk = opt_int("LJMD_WALK_CHUNK");
    k.vanhove_chunk = opt_int("LJMD_VANHOVE_CHUNK");
    k.fp32_far_stream = flag("LJMD_FP32_FAR_STREAM", k.fp32_far_stream);
    k.fp32_vfar = flag("LJMD_FP32_VFAR", k.fp32_vfar);
    {
        const char *rs = std::getenv("LJMD_FP32_SPLIT");
        if (rs && *rs) k.fp32_split = std::max(0.0, std::atof(rs));
    }
    k.overlap_exchange = flag("LJMD_OVERLAP_EXCHANGE", k.overlap_exchange);
    k.migrate_blocks = is("LJMD_MIGRATE_DEAL", "blocks");
    {
        const char *xm = std::getenv("LJMD_MULTI_EXCHANGE");
        k.multi_exchange = xm ? xm : "";
    }
    k.multi_migrate_every = std::max(0, env_int("LJMD_MULTI_MIGRATE_EVERY", k.multi_migrate_every));
    k.multi_threads = flag("LJMD_MULTI_THREADS", k.multi_threads);
    k.batch_group_streams = !is("LJMD_BATCH_GROUP_STREAMS", "0");
    k.batch_rhok_waves = env_int("LJMD_BATCH_RHOK_WAVES", k.batch_rhok_waves);
    return k;
}

void scalars_from_sums(double s12, double s6, double kx, double ky, double kz, double te, double td, double tdd,
                       double *epot, double *ekin, double *d_epot, double *dd_epot)
{
    if (epot) *epot = 4.0 * (s12 - s6) + te;                          // lj_potential_energy.f90:140,:188,:221
    if (d_epot) *d_epot = 24.0 * (-2.0 * s12 + s6) + td;              // :143,:177,:192,:222
    if (dd_epot) *dd_epot = 24.0 * (26.0 * s12 - 7.0 * s6) + tdd;     // :178,:193,:223
    if (ekin) *ekin = 0.5 * (kx + ky + kz);                           // verlet.f90:93-95
}

namespace {
void neg192(uint64_t (&x)[3])
{
    x[0] = ~x[0]; x[1] = ~x[1]; x[2] = ~x[2];
    const uint64_t one[3] = {1, 0, 0};
    add192(x, one);
}

// x k mod 2^192 (k > 0): two's complement wraps consistently, the admissible range never gets near the bound
void scale192(uint64_t (&x)[3], uint64_t k)
{
    unsigned __int128 carry = 0;
    for (int w = 0; w < 3; ++w) {
        const unsigned __int128 p = (unsigned __int128)x[w] * k + carry;
        x[w] = (uint64_t)p;
        carry = p >> 64;
    }
}

// arithmetic shift right by one (the ordered-pair sums are even: u^6_ij and u^6_ji have the same bits)
void half192(uint64_t (&x)[3])
{
    x[0] = (x[0] >> 1) | (x[1] << 63);
    x[1] = (x[1] >> 1) | (x[2] << 63);
    x[2] = (uint64_t)((int64_t)x[2] >> 1);
}
}  // namespace

void scalars_from_exact_sums(const uint64_t (&ordered)[5][3], double te, double td, double tdd, bool have_e, bool have_k,
                             double *epot, double *ekin, double *d_epot, double *dd_epot)
{
    uint64_t sum[5][3];
    std::memcpy(sum, ordered, sizeof sum);
    half192(sum[0]);                             // ordered -> unordered pairs
    half192(sum[1]);
    const double nan = std::numeric_limits<double>::quiet_NaN();
    if (epot) {                                  // 4 R(S12 - S6) + tail_e
        uint64_t x[3] = {sum[1][0], sum[1][1], sum[1][2]};
        neg192(x);
        add192(x, sum[0]);
        *epot = have_e ? 4.0 * fixed_to_double(x) + te : nan;
    }
    if (d_epot) {                                // 24 R(S6 - 2 S12) + tail_d
        uint64_t x[3] = {sum[0][0], sum[0][1], sum[0][2]};
        scale192(x, 2);
        neg192(x);
        add192(x, sum[1]);
        *d_epot = have_e ? 24.0 * fixed_to_double(x) + td : nan;
    }
    if (dd_epot) {                               // 24 R(26 S12 - 7 S6) + tail_dd
        uint64_t x[3] = {sum[0][0], sum[0][1], sum[0][2]}, y[3] = {sum[1][0], sum[1][1], sum[1][2]};
        scale192(x, 26);
        scale192(y, 7);
        neg192(y);
        add192(x, y);
        *dd_epot = have_e ? 24.0 * fixed_to_double(x) + tdd : nan;
    }
    if (ekin) {                                  // 0.5 ((Kx + Ky) + Kz)
        const double kx = fixed_to_double(sum[2]), ky = fixed_to_double(sum[3]), kz = fixed_to_double(sum[4]);
        *ekin = have_k ? 0.5 * ((kx + ky) + kz) : nan;
    }
}

}  // namespace ljmdh
