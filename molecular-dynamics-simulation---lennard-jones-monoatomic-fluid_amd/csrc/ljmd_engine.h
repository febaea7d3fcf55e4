// ljmd_engine.h -- the engine object behind the opaque ljmd_t of include/ljmd.h, its launch plan (ljmd_plan.cpp) and the
// internal functions the C ABI (ljmd_capi.cpp, ljmd_profile.cpp, ljmd_stateless.cpp) and the single-process multi-device
// driver (ljmd_multi.cpp) share: step phases (ljmd_engine.cpp), memory and transfers (ljmd_storage.cpp), record
// combination (ljmd_records.cpp), ownership migration (ljmd_migrate.cpp).
#ifndef LJMD_ENGINE_H
#define LJMD_ENGINE_H

#include "ljmd_common.h"

#include <rccl/rccl.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <mutex>
#include <vector>

#include "ljmd_internal.h"
#include "ljmd_resident.h"
#include "ljmd_sort.h"

using namespace ljmdk;

namespace ljmdh {

constexpr unsigned kRingCap = 4096;     // per-step partial records kept on the device
constexpr int kTargetWorkgroups = 2048; // >> 256 CUs (8 per CU) for the pair kernels
constexpr int kXcdMinGroups = 256;      // row groups per rank from which the XCD-aware work mapping is used (neutral below)
constexpr int kMixedMinN = 16384;       // smallest system the mixed-precision mode accepts
constexpr long kN3ItemsFor4 = 6000;     // (row group, offset) pairs a rank needs before 4 (n >= 32768 on one rank) ...
constexpr long kN3ItemsFor2 = 1000;     // ... or 2 (n >= 6144) tiles per row group pay off: profiles/r04_unit_sweep.txt
constexpr long kN3LargeItems = 131072;  // (row group, offset) pairs of a rank from which work items are slices of whole offsets
constexpr int kN3MidTargetItems = 32768;   // work items aimed at below that on one rank (units of one pass)
constexpr int kBothTiesMaxGroups = 128; // row groups up to which the tie d = NG / 2 is worked from both sides
constexpr int kFuseTailMaxRowTiles = 2; // tiles per row group up to which small systems take the two-launch step ...
constexpr int kFuseTailMaxN = 20000;    // ... and their largest particle count (n = 24 576: the in-kernel pass descriptors cost the pair kernel more than the launches save)
constexpr int kReduceSplitMinN = 131072;   // one rank, fp64: from here the slab reduction runs in two phases (LaunchPlan::split_s1) ...
constexpr int kReduceSplitShare = 8;       // ... with 1 / this of the pair kernel's slices in the second launch (profiles/reduce_split_sweep.txt)
constexpr int kMaxProfiledLaunches = 4096;
constexpr int kEventsPerLaunch = 9;

struct EventSet {
    // 0: before K1, 1: before geometry, 2: before pair, 3: after pair, 4: end (engine stream);
    // 5 / 6: around the position exchange, 7 / 8: around the force exchange, on the stream that carries them
    hipEvent_t e[kEventsPerLaunch];
    bool has_pos_x = false, has_force_x = false;   // events 5 / 6 and 7 / 8 were recorded for this launch
};

// What plan_engine decides from (parameters, n, n_ranks, precision mode, knobs) when the engine is created; constant
// afterwards.
struct LaunchPlan {
    int S = 0, P = 0;                 // particles of the shard, and padded to kSlotAlign
    int TB = 0, T = 0, W = 0;         // tiles of the shard, of all ranks, 64-bit mask words per tile row
    bool rc_allows_fast = false;      // rc <= (1 - 1e-9) * L/2
    bool sort_enabled = true;
    int resort_every = 20;
    // k-d ordering (default): per level the segment boundaries in particle units
    std::vector<int> kd_level_nseg;       // segments at level l
    std::vector<size_t> kd_level_off;     // offset of level l's boundaries inside kd_offsets
    std::vector<int> kd_offsets;          // uploaded to d_kd_offsets
    int kd_finish_from = 0;               // levels below this one take the library sort, it and the later ones
                                          // kd_finish_kernel (ljmd_sort.h); = number of levels: none does (LJMD_KD_SORT=cub)
    int nslab_g = 1, chunk_g = 0;     // generic kernel: grid (P/256, nslab_g), chunk_g j per slice
    int nslab_t = 1, chunk_t = 0;     // tile kernel:    grid (TB/4, nslab_t), chunk_t column tiles per slice
    // Newton-3 kernel (single rank): NG row groups, offsets 0..Dmax in nslab_n slices of dchunk
    bool use_n3 = false;
    int wg_waves = 1;                 // LJMD_N3_WG_WAVES: row groups (waves) per pair-kernel workgroup (1, 2, 4)
    bool both_ties = false;           // one rank, one wave per workgroup: the tie d = NG / 2 is worked from both sides (N3Args::both_ties)
    int uchunk = 0;                   // units (passes) per work item (N3Args::uchunk)
    int CS = 0, CS2 = 0, j_by_group = 0;   // slab_j / slab_j2: blocks per column tile, block numbering (N3Args::slab_j)
    int NG = 0, NGo = 0, Dmax = 0, nslab_n = 1, dchunk = 0;
    int rt = kRowTiles;               // tiles per row group (LJMD_N3_ROW_TILES; auto: 4, or 2 / 1 for small systems)
    // LJMD_FUSE_TAIL (default on): small single-rank systems run a step as TWO launches -- the pair kernel with its pass
    // descriptors worked out in-kernel, and tile_tail_kernel (slab reduction + kick + step record + the NEXT step's K1)
    bool fuse_tail = false;
    // LJMD_REDUCE_SPLIT: the pair kernel runs the slices [0, split_s1) and [split_s1, nslab_n) in two launches, and the slab
    // reduction sums what the first one completed -- those row-side slices and the blocks j < split_j1 of every column tile --
    // beside the second (enqueue_pair_forces).  0 = one launch, one-phase reduction
    int split_s1 = 0, split_j1 = 0;
    int nslab_max = 1, n_wg_max = 0;  // slices of d_slab, workgroup partials of d_wg_part: the largest of the kernel families
    int n_ke = 0;
};

// the rejection "LJMD_PRECISION_FP32_FORCE needs the Newton-3 path and n >= kMixedMinN" is the planner's
int plan_engine(const SimParams &sim, int n, int n_ranks, int precision_mode, const Knobs &k, LaunchPlan *out);

}  // namespace ljmdh

struct ljmd_multi;

using namespace ljmdh;

struct ljmd : ljmdh::SimParams {      // parameters (type(sim_params), md_types.f90:27-50): derive_params
    // single-process multi-device parent (ljmd_create_multi, ljmd_multi.cpp): owns one child engine per device
    // and no device memory of its own; every public entry point dispatches on it
    ljmd_multi *multi = nullptr;
    bool poisoned = false;            // a batch of steps failed half-way: LJMD_ERR_STATE until ljmd_set_state
    int inject_failure_at = -1;       // LJMD_INJECT_FAILURE_AT_STEP (fault injection for the tests): the force phase of the
                                      // evaluation with this index fails once, behind an already enqueued drift
    int n = 0, rank = 0, G = 1, device = 0, mode = 0;
    ljmdh::Knobs knobs;               // the environment as of ljmd_create
    ljmdh::LaunchPlan plan;           // constant after ljmd_create
    bool tail_on = true;              // ljmd_set_tail_corrections (the reference's use_tail_corrections, default .true.)
    bool positions_compact = false;   // coordinate spread < 2.4 L (always true after a wrap)
    bool positions_wide = false;      // coordinate spread >= 1.4 L: tile_boxes_kernel frames the wrapped coordinates (never after a wrap)
    bool have_state = false, have_accel = false;
    int steps_since_sort = 0;

    hipStream_t stream = nullptr;
    ncclComm_t comm = nullptr;        // RCCL communicator over the G ranks (multi-GPU only)
    // position all-gather overlapped with the velocity half-kick: the collective runs on comm_stream between
    // ev_pos_ready (positions drifted, engine stream) and ev_gather_done (awaited by the engine stream)
    hipStream_t comm_stream = nullptr;
    hipEvent_t ev_pos_ready = nullptr, ev_gather_done = nullptr;
    bool gather_done_for_step = false;
    // ---- HBM-resident state (layout: ljmd_internal.h) ----
    double *d_pos = nullptr;      // [G][3][P] exchange buffer (all positions)
    double *d_ru = nullptr, *d_v = nullptr, *d_a = nullptr;   // [3][P]
    double *d_slab = nullptr;     // [nslab_max][3][P]
    double *d_wg_part = nullptr;  // [n_wg_max][2]
    double *d_fold = nullptr;     // [kFoldBlocks][2]
    unsigned *d_ticket = nullptr; // blocks-done counter of the kick kernel with the finalize folded in
    bool want_energy = true;      // false: the next force evaluations skip the energy sums (epot, d_epot, dd_epot = NaN)
    // the two-launch step (LaunchPlan::fuse_tail).
    // kick_hint / next_drift_hint: what the caller of enqueue_pair_forces already knows about the rest of the step (-1 = not
    // known: the split-phase API); reduce_deferred: the pair phase left the reduction to the tail launch of enqueue_kick;
    // drift_prefused: the previous step's tail has already run this step's K1
    int kick_hint = -1;
    bool next_drift_hint = false;
    bool reduce_deferred = false, deferred_n3 = false;
    int deferred_nslab = 0;
    bool drift_prefused = false;
    double *d_ke_tile = nullptr;      // [T][3] per-tile sums of v^2
    bool boxes_valid = false;     // d_bbox already holds the boxes of the current positions (written by the drift kernel)
    double *d_ke_part = nullptr;  // [n_ke][3]
    double *d_ring = nullptr;     // [kRingCap][rec_stride] (reproducible mode: int64 words)
    int rec_stride = kPartialStride;  // 8-byte words per step record: kPartialStride, or kExactWords in the reproducible mode
    // reproducible mode (LJMD_PRECISION_FP64_REPRODUCIBLE, ljmd_internal.h: FixedArgs)
    __int128 *d_fslab = nullptr;  // [nslab_t][kFixedQuantities][P]
    unsigned *d_fflag = nullptr;  // [nslab_t][TB]
    int64_t *d_fblk = nullptr;    // [P / kBlock][kExactWords]
    int64_t *d_frec = nullptr;    // [kExactWords]: the record of ljmd_kinetic_energy
    bool pending_energy = true;   // the pending pair evaluation summed u^6, u^3
    unsigned *d_ring_pos = nullptr;
    double *d_bbox = nullptr;     // [T][kBoxStride]
    uint64_t *d_mask = nullptr;   // [TB][W]
    double *d_pos_tc = nullptr;   // [G][3][P] tile-coherent copy of d_pos for the Newton-3 kernels (tile_boxes_kernel)
    unsigned *d_desc = nullptr;   // [NGo][T] pass descriptors of the Newton-3 kernel (tile_class_kernel)
    unsigned *d_desc_far = nullptr;   // same for the fp32 far kernel of the mixed mode (from mask_far)
    float *d_desc2 = nullptr;     // [NGo][T][8] direction + thresholds of the cluster passes (LJMD_N3_CLUSTERS, default on)
    // sorting scratch
    int *d_idx = nullptr, *d_idx2 = nullptr, *d_perm = nullptr, *d_perm2 = nullptr;
    double *d_tmp3 = nullptr;     // [3][P]
    double *d_ru2 = nullptr, *d_v2 = nullptr, *d_a2 = nullptr;   // [3][P]: a re-sort gathers into them and swaps each with its set
    void *d_cub = nullptr;
    size_t cub_bytes = 0;
    std::vector<int> kd_axis;             // k-d ordering: split axis of level l, always the longest remaining extent
    int *d_kd_offsets = nullptr;
    unsigned long long *d_kd_keys = nullptr, *d_kd_keys2 = nullptr;   // [P]

    unsigned ring_consumed = 0;   // host mirror: records already read back
    unsigned ring_issued = 0;     // host mirror: finalize launches issued
    // two launches per step, record fold off the critical path (tile_tail_kernel): the step's record is folded by the NEXT
    // tail launch of the batch; the workgroup partials and per-tile v^2 sums it reads alternate between two buffers
    bool fold_pending = false;
    ljmdk::FinalizeArgs pending_fold{};
    int fold_parity = 0;
    size_t wg_part_stride = 0;        // doubles per wg_part buffer
    double *d_slab_j = nullptr;
    unsigned char *d_flag_j = nullptr;
    // two-phase slab reduction (LaunchPlan::split_s1): the four waves' partial sums per tile, the stream of lowest priority
    // that carries the pair kernel's second launch, and the two events that fence it against the engine's stream
    double *d_red_part = nullptr;     // [TB][4][3][64]
    hipStream_t side_stream = nullptr;
    hipEvent_t ev_side_go = nullptr, ev_side_done = nullptr;
    // mixed precision (mode = LJMD_PRECISION_FP32_FORCE): far tile pairs in fp32
    uint64_t *d_mask_far = nullptr;
    double *d_slab_j2 = nullptr;
    unsigned char *d_flag_j2 = nullptr;
    // reduced raw accelerations: fpart [G or 1][3][P]; frecv [3][P] = reduce-scatter result (G > 1, Newton-3)
    double *d_fpart = nullptr, *d_frecv = nullptr;
    double *d_fall = nullptr;         // [G][3][P] blocks received in the all-to-all form of the force exchange
    bool forces_pending = false;      // pair kernel + slab reduction enqueued, kick not yet
    bool external_force_exchange = false;   // tests: the caller sums fpart over ranks into frecv
    int pending_n_wg = 0;
    double pending_scale = 0.5;

    double *h_stage = nullptr;    // pinned, 3*G*P doubles
    double *h_ring = nullptr;     // pinned, kRingCap records
    std::vector<int> h_perm;      // slot -> original local index (>= S on padding)
    bool perm_dirty = false;

    // asynchronous snapshot (ljmd_snapshot_begin/end): device copy of r, ru, v, a [4][3][P] + perm [P],
    // its pinned host mirror, the second stream that carries the HBM -> host transfer
    // mixed precision: the fp32 far pass runs on its own stream beside the fp64 near pass (LJMD_FP32_FAR_STREAM, default on)
    hipStream_t far_stream = nullptr;
    hipEvent_t ev_far_go = nullptr, ev_far_done = nullptr;
    hipStream_t copy_stream = nullptr;
    hipEvent_t ev_snap_ready = nullptr, ev_snap_done = nullptr;
    double *d_snap = nullptr, *h_snap = nullptr;
    int *d_snap_perm = nullptr, *h_snap_perm = nullptr;
    bool snap_in_flight = false;
    bool snap_ready = false;      // all of the above exist

    // Ownership migration (multi-GPU, ljmd_migrate.cpp: migrate_pack / migrate_deal).  gid0[j] = particle id -- global index in
    // the order of the last ljmd_set_state (or of the last rebase) -- of the particle at position j of this engine's arrays
    // (its "original order": what get_state returns and the slot permutation refers to); identity (rank S + j) until a deal
    int *d_gid0 = nullptr;            // [P]
    std::vector<int> h_gid0;          // host mirror, valid while `migrated`
    bool migrated = false;            // the shard is no longer the index range [rank S, (rank + 1) S) of the caller's arrays
    double *d_mig = nullptr;          // [G][kMigrateRows][P] migration buffer (lazy)
    int *d_mig_idx = nullptr, *d_mig_idx2 = nullptr;                    // [n] storage indices g P + s
    unsigned long long *d_mig_keys = nullptr, *d_mig_keys2 = nullptr;   // [n]
    int *d_mig_offsets = nullptr;
    void *d_mig_cub = nullptr;
    size_t mig_cub_bytes = 0;
    std::vector<int> mig_level_nseg, mig_axis;
    std::vector<size_t> mig_level_off;
    double mig_ext[3] = {0, 0, 0};    // extents of a rank's block after the deal (choose the shard's k-d axes)
    int32_t migrations = 0;

    // the resident observables (entry points and release_resident: ljmd_resident.cpp).  g(r) (ljmd_rdf_*, core
    // ljmd_rdf.cpp); a multi-device parent keeps only nbins here, the ranks own the buffers
    ljmdr::RdfState rdf;
    // MSD / VACF (ljmd_tcf_*, core ljmd_tcf.cpp): one-rank engines only
    ljmdt::TcfState tcf;
    // pressure tensor (ljmd_stress_*, core ljmd_stress.cpp); a multi-device parent keeps only max_snapshots and the
    // snapshot count here
    ljmds::StressState stress;
    // heat flux (ljmd_heatflux_*, core ljmd_heatflux.cpp): one-rank engines only
    ljmdq::HeatfluxState heatflux;
    // van Hove self-correlation (ljmd_vanhove_*, core ljmd_vanhove.cpp): one-rank engines only
    ljmdv::VanHoveState vanhove;
    // density modes (ljmd_rhok_*, core ljmd_rhok.cpp): one-rank engines only
    ljmdc::RhokState rhok;
    // current modes (ljmd_current_*, core ljmd_current.cpp): one-rank engines only
    ljmdc::CurrentState current;
    bool step_open = false;           // between ljmd_step_begin and ljmd_step_finish (split-phase API)

    bool profiling = false;
    std::vector<EventSet> ev_pool;
    size_t ev_used = 0;

    std::string err;
};


namespace ljmdh {

// the checks an entry point of the C ABI starts with, in this order; `who` is the public function's name
enum : unsigned { kHandle = 1, kHaveState = 2, kHaveAccel = 4, kNotPoisoned = 8 };
int entry_checks(const ljmd_t *h, const char *who, unsigned checks);

inline double *own_block(ljmd_t *h) { return h->d_pos + (size_t)h->rank * 3 * h->plan.P; }
inline bool needs_force_exchange(const ljmd_t *h) { return h->plan.use_n3 && (h->G > 1 || h->knobs.force_collectives); }
bool fast_path_ok(const ljmd_t *h);
IntegrateArgs integrate_args(ljmd_t *h);

// device and pinned host memory of a planned engine (h->plan), in the order and sizes of its kernels' layouts; on failure
// the caller releases whatever exists
int allocate_engine(ljmd_t *h);
void release(ljmd_t *h);
// what ljmd_rdf_configure, ljmd_tcf_configure, ljmd_stress_configure, ljmd_heatflux_configure, ljmd_vanhove_configure,
// ljmd_rhok_configure and ljmd_current_configure allocated; the engine's device is current
// (ljmd_resident.cpp; called by release)
void release_resident(ljmd_t *h);
// HBM -> host of any of r, ru, v, a (dsts[3 w + k], NULL = skip) and of the last n_records scalar records
int download_state(ljmd_t *h, double *const dsts[12], unsigned n_records);
int upload_shard3(ljmd_t *h, double *dst, const double *x, const double *y, const double *z);
int resort(ljmd_t *h, bool with_accel);
int refresh_perm(ljmd_t *h);
// the communication stream and its two fences against the engine's stream (ljmd_engine.cpp)
bool use_comm_stream(const ljmd_t *h);
int comm_begin(ljmd_t *h);
int comm_end(ljmd_t *h);
int allgather_on(ljmd_t *h, hipStream_t s);

// one MD step = enqueue_drift | position exchange (multi-rank) | enqueue_pair_forces | force exchange | enqueue_kick
int enqueue_drift(ljmd_t *h, EventSet *q);
// the same in two halves, for a caller that issues the position exchange itself between them (ljmd_multi.cpp):
// positions (+ re-sort on a re-sort step; *split = false then, and the velocity half-kick has already run) ...
int enqueue_drift_positions(ljmd_t *h, EventSet *q, bool *split);
// ... and the velocity half-kick, concurrent with the exchange
int enqueue_drift_velocities(ljmd_t *h);
int enqueue_pair_forces(ljmd_t *h, EventSet *q);
int enqueue_kick(ljmd_t *h, bool kick, EventSet *q);
// both phases from one caller; next_drift: another step follows in the same batch (its K1 may ride on this step's tail launch)
int enqueue_forces(ljmd_t *h, bool kick, EventSet *q, bool next_drift = false);
int fetch_ring(ljmd_t *h, unsigned count);
void combine_one(const ljmd_t *h, const double *recs, int n_ranks, double *epot, double *ekin, double *d_epot,
                 double *dd_epot);
inline bool reproducible(const ljmd_t *h) { return h->mode == LJMD_PRECISION_FP64_REPRODUCIBLE; }
// the reproducible mode's combination of n_ranks exact records (kExactWords each); LJMD_ERR_RANGE on a range flag
int combine_exact(const ljmd_t *h, const int64_t *recs, int n_ranks, double *epot, double *ekin, double *d_epot,
                  double *dd_epot);
// either mode: records of h->rec_stride words as fetch_ring leaves them; a range error poisons `poison`
int combine_records(ljmd_t *poison, const ljmd_t *h, const double *recs, int n_ranks, double *epot, double *ekin,
                    double *d_epot, double *dd_epot);
// reproducible mode: this engine's exact record of sum v^2 (Kx, Ky, Kz words) of the resident velocities
int kinetic_exact(ljmd_t *h, int64_t *rec /* [kExactWords] */);
EventSet *next_events(ljmd_t *h);
// ownership migration in three phases, all on the engine's stream: (1) the own block of the migration buffer <- ru, v, a,
// ids; (2) -- by the caller or the library -- all-gather of the G blocks (kMigrateRows * P doubles each; block g at
// migrate_buffer(h) + g * kMigrateRows * P); (3) the deal + the rank's new state (the exchange buffer must hold everybody's
// CURRENT positions).  Afterwards the position exchange has to run again.
int migrate_pack(ljmd_t *h);
double *migrate_buffer(ljmd_t *h);
int migrate_deal(ljmd_t *h);
// a caller that keeps the composite table itself (ljmd_multi.cpp): the ids start again at rank S + j
int migrate_rebase(ljmd_t *h);

}  // namespace ljmdh
#endif
