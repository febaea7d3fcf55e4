// ljmd_common.h -- what every host file of libljmd.so shares, whatever engine it serves: error reporting, the parameter
// guards and derived parameters of the reference's md_types.f90, the device probe, the table of environment knobs and the
// formulas that turn the summed pair terms into the four scalars.
#ifndef LJMD_COMMON_H
#define LJMD_COMMON_H

#include "ljmd.h"

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <optional>
#include <string>

namespace ljmdh {

extern thread_local std::string g_last_error;

// md_types.f90:22
constexpr double kPi = 3.1415926535897932384626433832795;

// formats the message into the thread's last error and, where there is one, into the handle's own `err`
int failv(std::string *handle_err, int code, const char *fmt, va_list ap);

inline int fail(std::nullptr_t, int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    failv(nullptr, code, fmt, ap);
    va_end(ap);
    return code;
}

// the message string itself, for code that sees no handle (the cores of the resident observables)
inline int fail(std::string *err, int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    failv(err, code, fmt, ap);
    va_end(ap);
    return code;
}

// H: any handle type with a std::string err (ljmd, ljmd_batch)
template <class H>
int fail(const H *h, int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    failv(h ? &const_cast<H *>(h)->err : nullptr, code, fmt, ap);
    va_end(ap);
    return code;
}

#define LJMD_HIP(h, call)                                                                   \
    do {                                                                                    \
        hipError_t e_ = (call);                                                             \
        if (e_ != hipSuccess)                                                               \
            return ljmdh::fail((h), LJMD_ERR_HIP, "%s failed: %s (%s:%d)", #call,           \
                               hipGetErrorString(e_), __FILE__, __LINE__);                  \
    } while (0)

#define LJMD_TRY(expr)                      \
    do {                                    \
        const int rc__ = (expr);            \
        if (rc__ != LJMD_OK) return rc__;   \
    } while (0)

inline int env_int(const char *name, int dflt)
{
    const char *v = std::getenv(name);
    return (v && *v) ? std::atoi(v) : dflt;
}

// the guards of md_types.f90:143-161 and allocate_state :192, in the reference's order; `who` prefixes the message
int check_sim_params(const char *who, int n, double box_length, double dt, double rc);

// a HIP device is present and `device` names one (after the caller's own guards: they need no device)
int probe_device(int device, const char *who);

// type(sim_params), md_types.f90:27-50, and what compute_derived_params (:137-159) and the tail corrections of
// lj_potential_energy.f90:205-223 derive from it
struct SimParams {
    double L = 0, invL = 0, volume = 0, rc = 0, rc2 = 0, dt = 0, dt_half = 0, dt_sq_half = 0;
    double tail_e = 0, tail_d = 0, tail_dd = 0;
};
SimParams derive_params(int n, double box_length, double dt, double rc);

// epot, d_epot, dd_epot from the unordered-pair sums of u^12 and u^6, ekin from the three sums of v^2 (NULL = not wanted)
void scalars_from_sums(double s12, double s6, double kx, double ky, double kz, double te, double td, double tdd,
                       double *epot, double *ekin, double *d_epot, double *dd_epot);

// The reproducible mode's form, shared by the engine (ljmd_records.cpp) and the batch engine: `ordered` holds the exact
// sums {S12, S6 over the ORDERED pairs, Kx, Ky, Kz}, signed 192-bit integers in units of 2^-64 as three little-endian
// limbs.  The pair sums are halved and combined as integers, then ONE rounding per scalar, then the tail constants.
// have_e / have_k false (the record carries no energy / kinetic sums): those scalars are NaN.
void scalars_from_exact_sums(const uint64_t (&ordered)[5][3], double te, double td, double tdd, bool have_e, bool have_k,
                             double *epot, double *ekin, double *d_epot, double *dd_epot);

// Every LJMD_* environment variable an engine reads, with its default.  read_knobs() is called once per engine, when it
// is created; the handle keeps the result, and a later change of the environment does not reach an existing engine.
// (The stateless drop-ins read LJMD_DEVICE, LJMD_REPRODUCIBLE and LJMD_STATELESS_FASTPATH per call: ljmd_stateless.cpp.)
struct Knobs {
    bool sort = true;                       // LJMD_SORT: spatial re-ordering (systems of >= 1024 particles)
    bool force_generic = false;             // LJMD_FORCE_GENERIC=1: always take the exact generic kernel (A/B tests)
    bool force_collectives = false;         // LJMD_FORCE_COLLECTIVES=1: a 1-rank engine still issues its RCCL calls (tests)
    bool fuse = true;                       // LJMD_FUSE: boxes inside the drift kernel, finalize inside the kick kernel
    bool fuse_tail = true;                  // LJMD_FUSE_TAIL: two launches per step for small single-rank systems
    bool fuse_defer_record = true;          // LJMD_FUSE_DEFER_RECORD: a step's record is folded by the next tail launch
    int xcd_remap = 4;                      // LJMD_N3_XCD_REMAP: consecutive row groups per XCD chunk (0 = plain mapping)
    int inject_failure_at_step = -1;        // LJMD_INJECT_FAILURE_AT_STEP: initial value of ljmd::inject_failure_at (tests)
    bool exchange_alltoall = false;         // LJMD_FORCE_EXCHANGE=alltoall: direct sends + local rank-order sum
    std::optional<int> resort_every;        // LJMD_RESORT_EVERY: steps between two re-sorts (unset: by system size)
    bool kd_sort_cub = false;               // LJMD_KD_SORT=cub: every k-d level of a re-sort takes the library sort (A/B tests)
    int n3_row_tiles = 0;                   // LJMD_N3_ROW_TILES: tiles per row group (1, 2, 4; else by system size)
    int n3_wg_waves = 0;                    // LJMD_N3_WG_WAVES: row groups per pair-kernel workgroup (1, 2, 4; else by slab size)
    int slab_budget_gb = 64;                // LJMD_SLAB_BUDGET_GB: column slab above which more waves share a workgroup
    bool n3_both_ties = true;               // LJMD_N3_BOTH_TIES: the tie d = NG / 2 worked from both sides
    int n3_min_n = 4096;                    // LJMD_N3_MIN_N: smallest system that takes the Newton-3 kernel
    bool n3 = true;                         // LJMD_N3
    std::optional<int> n3_target_waves;     // LJMD_N3_TARGET_WAVES: work items the pair kernel aims at (unset: by system size)
    bool n3_clusters = true;                // LJMD_N3_CLUSTERS: cluster passes (4-tile row groups, one wave per workgroup)
    bool n3_pertile = true;                 // LJMD_N3_PERTILE: per-tile periodic images in the geometry pre-pass
    std::optional<int> reduce_split;        // LJMD_REDUCE_SPLIT: slices of the pair kernel run in a second launch beside the slab
                                            // reduction's first phase (0 = one launch; unset: by system size)
    std::optional<int> walk_chunk;          // LJMD_WALK_CHUNK: column-tile steps per slice of the resident g(r) / pressure tensor /
                                            // heat flux walk, clamped to [1, steps] (tests; unset: by the grid rdf_plan_walk aims at)
    std::optional<int> vanhove_chunk;       // LJMD_VANHOVE_CHUNK: live origins per slice of the van Hove terms kernel, clamped to
                                            // [1, min(live origins, 128)] (tests; unset: by the grid vanhove_plan_slices aims at)
    bool fp32_far_stream = true;            // LJMD_FP32_FAR_STREAM: the fp32 far pass on a stream of its own
    bool fp32_vfar = true;                  // LJMD_FP32_VFAR: the very-far form of the fp32 kernel
    double fp32_split = 5.0;                // LJMD_FP32_SPLIT: boxes closer than this stay fp64
    bool overlap_exchange = true;           // LJMD_OVERLAP_EXCHANGE: exchanges on a communication stream
    bool migrate_blocks = false;            // LJMD_MIGRATE_DEAL=blocks (default slabs)
    std::string multi_exchange;             // LJMD_MULTI_EXCHANGE: rccl, copy or host ("" = by the device list)
    int multi_migrate_every = 2000;         // LJMD_MULTI_MIGRATE_EVERY: steps between two ownership migrations (0 = never)
    bool multi_threads = true;              // LJMD_MULTI_THREADS: one host thread per rank for the step loop
    bool batch_group_streams = true;        // LJMD_BATCH_GROUP_STREAMS=0: the batch engine's groups one after another
    int batch_rhok_waves = 0;               // LJMD_BATCH_RHOK_WAVES: waves per workgroup of the batch density modes kernel
                                            // (2, 4, 8; else the built-in choice: tools/batch_rhok_rate.py)
};
Knobs read_knobs();

}  // namespace ljmdh
#endif
