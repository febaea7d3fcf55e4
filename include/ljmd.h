/*
 * ljmd.h -- C ABI of libljmd.so: the MI355X (gfx950) drop-in for the reference's
 * Lennard-Jones force/energy + velocity-Verlet hot path.
 *
 * The reference (Ledicia/Molecular-Dynamics-Simulation---Lennard-Jones-monoatomic-fluid)
 * has no FFI layer; its operator boundary is two Fortran module procedures
 *     compute_lj_potential_energy(params, state, epot, d_epot, dd_epot)
 *                                        scripts/physics/lj_potential_energy.f90:46
 *     verlet_step(params, state, epot, ekin, d_epot, dd_epot)
 *                                        scripts/physics/verlet.f90:41
 * plus the caller-side per-step unwrapped-coordinate update
 *                                        scripts/md_simulation_program.f90:339-353.
 * Derived types with allocatable components are not bind(C)-interoperable, so the
 * arrays cross as raw `double*` (c_loc(state%rx) ...) and the scalars by value.
 * INTEGRATION.md shows the ISO_C_BINDING stub that binds each entry point.
 *
 * Conventions
 *   - every function returns LJMD_OK (0) or a negative ljmd_status; the text of the
 *     last error is available from ljmd_last_error() (the Fortran shim turns a
 *     non-zero status into `stop 'ljmd: ...'`, the reference's own convention,
 *     e.g. lj_potential_energy.f90:77-82).
 *   - all arrays are fp64, length n, structure-of-arrays, 0-based in C.
 *   - one handle = one simulation on one GPU; a handle is not thread-safe
 *     (the reference is serial), independent handles may coexist.
 *   - there is NO CPU fallback: without a usable HIP device every compute entry
 *     point fails with LJMD_ERR_NO_DEVICE.
 */
#ifndef LJMD_H
#define LJMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ljmd ljmd_t;

typedef enum ljmd_status {
    LJMD_OK = 0,
    LJMD_ERR_INVALID_ARG = -1, /* a guard of md_types.f90:143-161 / lj_potential_energy.f90:77-82 failed */
    LJMD_ERR_NO_DEVICE = -2,   /* no HIP device / device code cannot run */
    LJMD_ERR_HIP = -3,         /* a HIP runtime call failed */
    LJMD_ERR_STATE = -4,       /* call sequence error (e.g. step before set_state), or a handle poisoned by a
                                  batch of steps that failed half-way: ljmd_set_state makes it usable again */
    LJMD_ERR_ALLOC = -5,
    LJMD_ERR_RANGE = -6        /* reproducible mode: a term was not finite or |term| >= 2^40 (a pair closer than about
                                  0.12 sigma, |v| >= 2^20); the handle is poisoned as after a failed batch */
} ljmd_status;

/* precision_mode for ljmd_create */
#define LJMD_PRECISION_FP64 0       /* all arithmetic fp64 (BASELINE configs 1-4)            */
#define LJMD_PRECISION_FP32_FORCE 1 /* mixed: pairs of tiles farther apart than r_split (env
                                       LJMD_FP32_SPLIT, default 5 sigma; 0 = all but the own row group) in
                                       fp32 tile-relative arithmetic, nearer pairs in fp64; fp64 accumulation
                                       and integrator.  Needs n >= 16384.  BASELINE config 5.             */
/*
 * LJMD_PRECISION_FP64_REPRODUCIBLE: results that are a function of the particle set alone -- bitwise independent of
 * input order, of the number of ranks (both multi-GPU forms), of re-sorting, of every tiling knob and of the launch
 * form, and bitwise equal to a CPU model of this definition (tests/reproducible_model.py).
 *   Per ordered pair (i, j), j != i, the reference's arithmetic (lj_potential_energy.f90:109-183): minimum image with
 *   round (half away from zero), r2 = (dx*dx + dy*dy) + dz*dz, r2 < rc2, u = 1/r2 (IEEE divide), u3 = (u*u)*u,
 *   u6 = u3*u3, m = 2*u6 - u3, fx = (m*dx)*u; no contraction.  With Q(t) = RNE(t 2^64), an exact integer, and R one
 *   round-to-nearest-even conversion to fp64:
 *     a_x(i)  = 24 R(2^-64 sum_j Q(fx_ij))                          (and y, z)
 *     S12 = sum_{i<j} Q(u6_ij),  S6 = sum_{i<j} Q(u3_ij)             (exact integers)
 *     epot    =  4 R(2^-64 (S12 - S6))       + tail_e
 *     d_epot  = 24 R(2^-64 (S6 - 2 S12))     + tail_d
 *     dd_epot = 24 R(2^-64 (26 S12 - 7 S6))  + tail_dd
 *     ekin    = 0.5 ((Kx + Ky) + Kz),  Kx = R(2^-64 sum_i Q(vx_i * vx_i))
 *   The integrator is the fp64 mode's.  Range: every term must be finite with |t| < 2^40, else the call that returns
 *   the step's results fails with LJMD_ERR_RANGE (never a silent wrap-around); n <= 2^23.  Per-particle sums are
 *   128-bit, totals 192-bit.  The gather (full-matrix) pair kernel: no Newton-3 form, no fused two-launch step.
 */
#define LJMD_PRECISION_FP64_REPRODUCIBLE 2
/* Exact per-rank step record of the reproducible mode (ljmd_read_partials_exact): five signed 192-bit integers as
 * three little-endian 64-bit limbs each -- {S12, S6} over this rank's ORDERED pairs, {Kx, Ky, Kz} over its
 * particles, all in units of 2^-64 -- then one flags word (1 = range error, 2 = forces-only step: no S12 / S6,
 * 4 = no second half-kick: no Kx / Ky / Kz). */
#define LJMD_EXACT_PARTIAL_WORDS 16

/* Which state array: argument of ljmd_device_ptr / selectors of get_state. */
enum { LJMD_R = 0, LJMD_RU = 1, LJMD_V = 2, LJMD_A = 3 };
#define LJMD_PARTIAL_STRIDE 8

/* ---- library-level ------------------------------------------------------ */

/* "ljmd <version> gfx950"; never NULL. */
const char *ljmd_version(void);
/* Number of visible HIP devices (0 when there is none); never fails. */
int32_t ljmd_device_count(void);
/* Text of the most recent error on this handle (h == NULL: the most recent
 * error of a failed ljmd_create or of a stateless call on this thread). */
const char *ljmd_last_error(const ljmd_t *h);

/* ---- handle lifecycle --------------------------------------------------- */

/*
 * Creates an engine for n particles in a cubic box.  Replaces init_params +
 * compute_derived_params + init_state (scripts/base/md_types.f90:105-201): the
 * derived constants 1/L, L**3, rc*rc, 0.5*dt, (0.5*dt)*dt are computed on the
 * host exactly as written there, and the same guards apply (n > 0, L > 0,
 * rc > 0, rc < L/2, dt > 0) -> LJMD_ERR_INVALID_ARG.
 * rank/n_ranks select the contiguous particle shard [rank*n/n_ranks,
 * (rank+1)*n/n_ranks) this engine integrates and owns pair rows for (SURVEY
 * 8(e)); n_ranks = 1 is the ordinary single-GPU engine.  n must be divisible
 * by n_ranks.
 */
int ljmd_create(ljmd_t **out, int32_t n, double box_length, double dt, double rc,
                int32_t precision_mode, int32_t device, int32_t rank, int32_t n_ranks);
void ljmd_destroy(ljmd_t *h);

/*
 * ONE host process, n_gpus devices (the thin Fortran driver's way to BASELINE config 4: N = 1 048 576 sharded
 * over the 8 GPUs of a node; the reference's caller loop md_simulation_program.f90:300-391 stays as it is).
 * The returned handle is used with the SAME entry points as a single-GPU handle -- ljmd_set_state / set_accel /
 * set_unwrapped / get_state, ljmd_compute_forces, ljmd_verlet_steps, ljmd_enqueue_steps / collect_steps,
 * ljmd_snapshot_begin / end, ljmd_kinetic_energy, ljmd_synchronize, ljmd_profile_*, ljmd_destroy -- with global
 * (length-n) arrays; inside, rank g = one engine on devices[g] (NULL = devices 0 .. n_gpus-1) integrating particles
 * [g n/n_gpus, (g+1) n/n_gpus), and per step one all-gather of the position blocks and (Newton-3) one
 * reduce-scatter of the partial accelerations, stream-ordered with no host synchronisation: RCCL over xGMI
 * (ncclCommInitAll; the collectives of all ranks grouped from the one host thread), or peer-to-peer copies +
 * a rank-ordered sum when LJMD_MULTI_EXCHANGE=copy or a device is listed more than once (RCCL refuses two ranks
 * on one device; this is how several ranks are rehearsed on one card).  The split-phase functions below
 * (ljmd_step_begin ...) are for the one-process-per-GPU form and return LJMD_ERR_STATE on such a handle.
 * n must be divisible by n_gpus.
 */
int ljmd_create_multi(ljmd_t **out, int32_t n, double box_length, double dt, double rc,
                      int32_t precision_mode, int32_t n_gpus, const int32_t *devices);

/* ---- state transfer ------------------------------------------------------ */

/* Host -> HBM.  Replaces read_rv_init + `ru <- r` (md_simulation_program.f90:221-231).
 * Accelerations are zeroed (init_state semantics). All six pointers required. */
int ljmd_set_state(ljmd_t *h, const double *rx, const double *ry, const double *rz,
                   const double *vx, const double *vy, const double *vz);
/* Host -> HBM for a / ru, so that a caller can resume from a full rva.dat snapshot or
 * run verlet_step on caller-owned accelerations (strict drop-in mode). NULL = keep. */
int ljmd_set_accel(ljmd_t *h, const double *ax, const double *ay, const double *az);
int ljmd_set_unwrapped(ljmd_t *h, const double *ux, const double *uy, const double *uz);
/* HBM -> host; any pointer may be NULL (skipped).  r, ru, v, a as in the four
 * records of an rva.dat snapshot (md_simulation_program.f90:384-387). */
int ljmd_get_state(ljmd_t *h, double *rx, double *ry, double *rz,
                   double *ux, double *uy, double *uz,
                   double *vx, double *vy, double *vz,
                   double *ax, double *ay, double *az);

/* ---- the hot path -------------------------------------------------------- */

/*
 * = compute_lj_potential_energy (lj_potential_energy.f90:46-225) on the resident
 * positions: overwrites the resident accelerations, returns epot, d_epot, dd_epot
 * including the x4 / x24 prefactors (:188-193) and the tail corrections (:205-223).
 */
int ljmd_compute_forces(ljmd_t *h, double *epot, double *d_epot, double *dd_epot);

/*
 * = nsteps x { verlet_step (verlet.f90:41-97) ; unwrapped update
 * (md_simulation_program.f90:339-353) } with no host synchronisation inside.
 * Requires valid resident accelerations (ljmd_compute_forces or ljmd_set_accel
 * first, as the reference's drivers do at md_simulation_program.f90:236).
 * epot/ekin/d_epot/dd_epot: each NULL or an array of nsteps doubles receiving the
 * value after every step.  With epot, d_epot and dd_epot all NULL nobody reads the
 * potential-energy sums and the steps run the forces-only pair kernel (see
 * ljmd_enqueue_steps_sampled); the trajectory is bit-for-bit the same.
 */
int ljmd_verlet_steps(ljmd_t *h, int32_t nsteps,
                      double *epot, double *ekin, double *d_epot, double *dd_epot);

/*
 * Asynchronous form of the production loop (md_simulation_program.f90:300-391), so that the
 * host's snapshot I/O (:374-387) overlaps the GPU's next steps instead of stalling them:
 *
 *   ljmd_enqueue_steps(h, k)      k Verlet steps on the engine's stream; returns at once.
 *                                 At most LJMD_MAX_PENDING_STEPS steps may be pending.
 *   ljmd_collect_steps(h, k, ..)  waits for the engine's stream and returns the scalars of the
 *                                 last k enqueued steps (arrays of k doubles or NULL).
 *   ljmd_snapshot_begin(h)        stream-ordered copy of r, ru, v, a (and the slot order) into
 *                                 a device snapshot buffer -- a few microseconds behind the
 *                                 steps enqueued so far -- then HBM -> pinned host on a SECOND
 *                                 stream; returns at once.  Steps enqueued afterwards run
 *                                 concurrently with that transfer and do not alter the snapshot.
 *   ljmd_snapshot_end(h, ...)     waits for the transfer only (not for the engine's stream) and
 *                                 delivers the twelve arrays as ljmd_get_state does.
 * One snapshot may be in flight at a time (LJMD_ERR_STATE otherwise).
 */
#define LJMD_MAX_PENDING_STEPS 4096
int ljmd_enqueue_steps(ljmd_t *h, int32_t nsteps);
/* As ljmd_enqueue_steps, for a segment of which only the LAST step is sampled -- the reference reads epot, d_epot,
 * dd_epot only where mod(step, output_interval) == 0 (md_simulation_program.f90:361; output_interval = 100 in the
 * reference's input file) although lj_potential_energy.f90 sums them on every call.  The pair kernel of the other
 * nsteps - 1 steps leaves the two energy sums out (forces-only instantiation, -6 % kernel time at n = 262144);
 * positions, velocities, accelerations and ekin are bit-for-bit those of ljmd_enqueue_steps, and ljmd_collect_steps
 * returns NaN for epot, d_epot, dd_epot of the steps that were not sampled. */
int ljmd_enqueue_steps_sampled(ljmd_t *h, int32_t nsteps);
/* The same switch for the phase API of a sharded engine (ljmd_step_begin / ljmd_step_forces / ljmd_step_finish):
 * on = 0 makes the following force evaluations forces-only until it is switched on again (default on).
 * ljmd_compute_forces always evaluates the sums. */
int ljmd_set_observables(ljmd_t *h, int32_t on);
int ljmd_collect_steps(ljmd_t *h, int32_t nsteps,
                       double *epot, double *ekin, double *d_epot, double *dd_epot);
int ljmd_snapshot_begin(ljmd_t *h);
int ljmd_snapshot_end(ljmd_t *h, double *rx, double *ry, double *rz,
                      double *ux, double *uy, double *uz,
                      double *vx, double *vy, double *vz,
                      double *ax, double *ay, double *az);

/* Kinetic energy of the resident velocities, one fused sum as at
 * md_simulation_program.f90:238-240 (t = 0 only). */
int ljmd_kinetic_energy(ljmd_t *h, double *ekin);

/* ---- stateless drop-ins (what the Fortran shim modules bind) ------------- */

/*
 * Exact signature-level replacement of compute_lj_potential_energy: host arrays in,
 * host arrays out, the params fields passed by value.  Internally keeps one cached
 * engine per (n, L, rc) on device 0; LJMD_REPRODUCIBLE=1 in the environment makes it a
 * LJMD_PRECISION_FP64_REPRODUCIBLE engine.
 */
int ljmd_compute_lj_potential_energy(int32_t n, double box_length, double rc,
                                     const double *rx, const double *ry, const double *rz,
                                     double *ax, double *ay, double *az,
                                     double *epot, double *d_epot, double *dd_epot);
/* Exact replacement of verlet_step: the nine state arrays are updated in place. */
int ljmd_verlet_step(int32_t n, double box_length, double dt, double rc,
                     double *rx, double *ry, double *rz,
                     double *vx, double *vy, double *vz,
                     double *ax, double *ay, double *az,
                     double *epot, double *ekin, double *d_epot, double *dd_epot);
/*
 * Trajectory analysis pair pass: adds the ordered-pair distance histogram of ONE
 * snapshot to hist[nbins] -- the O(n^2) loop of compute_rdf (scripts/md_one_run_analysis.py:556-584:
 * d -= L*rint(d/L), r = sqrt(.), bin = int(r / (rmax/nbins)) for r < rmax; every unordered pair
 * counts 2, exactly as the reference's np.add.at(hist, bins, 2.0)).  Integer counts, bit-exact.
 * Host arrays in; device 0.  nbins <= 8192.
 */
int ljmd_rdf_histogram(int32_t n, const double *x, const double *y, const double *z, double box_length,
                       int32_t nbins, double rmax, uint64_t *hist);
/*
 * Trajectory analysis, time-origin averages: MSD(lag) = < |ru(t0 + lag) - ru(t0)|^2 > (kind 0, arrays =
 * unwrapped positions) or VACF(lag) = < v(t0) . v(t0 + lag) > (kind 1, arrays = velocities) over particles and time
 * origins t0 = 0, origin_stride, ..., exactly as compute_msd_tau_timeorig / compute_vacf_tau_timeorig do
 * (scripts/md_one_run_analysis.py:404-489): per (origin, lag) the particle mean on the GPU (the reference's per-element
 * expressions; fixed summation order, equal to numpy's pairwise mean to rounding), the origins added on the host in the
 * reference's order.  x, y, z: [n_snap][n] host arrays; out: [min(max_lag, n_snap - 1) + 1].  n_snap >= 2.
 */
int ljmd_time_origin_average(int32_t kind, int32_t n_snap, int32_t n, const double *x, const double *y, const double *z,
                             int32_t max_lag, int32_t origin_stride, double *out);
/* The stateless entry points keep one cached engine (device LJMD_DEVICE, default 0).  ljmd_verlet_step
 * remembers the nine arrays it handed back; when the next call passes the same bytes again (the reference's
 * loop only reads them between steps) the resident state is stepped directly -- no upload, no spatial re-sort,
 * only the download (LJMD_STATELESS_FASTPATH=0 disables the check).  This frees the cached engine. */
void ljmd_stateless_reset(void);

/* ---- multi-GPU split-phase API (one process per GPU) -------- */

/* [i0, i1) = particle rows this engine owns -- until an ownership migration (ljmd_migrate) after ljmd_set_state: from then on it
 * owns the set ljmd_particle_ids names and this call fails with LJMD_ERR_STATE. */
int ljmd_shard_range(const ljmd_t *h, int32_t *i0, int32_t *i1);
/*
 * Device address of the exchange buffer holding ALL n positions in shard-blocked
 * SoA order: block g (g = 0..n_ranks-1) is x[P] y[P] z[P] of rank g's particles in
 * rank g's current (spatially sorted) slot order, P = n/n_ranks rounded up to a
 * multiple of 256, padding slots = NaN.  Rank g's own block is at offset g*3*P
 * doubles, so one in-place RCCL all-gather of 3*P doubles per rank refreshes it.
 */
void *ljmd_exchange_buffer(ljmd_t *h, int64_t *n_doubles_total, int64_t *own_offset_doubles,
                           int64_t *own_count_doubles);
/* Device address of one resident state array (LJMD_R..LJMD_A, axis 0..2), P slots in
 * the current device slot order; for zero-copy views (e.g. torch via __cuda_array_interface__). */
void *ljmd_device_ptr(ljmd_t *h, int32_t which, int32_t axis);
/*
 * RCCL exchange over xGMI.  Rank 0 obtains an id (ncclGetUniqueId) and ships the
 * LJMD_COMM_ID_BYTES to every rank by any out-of-band channel (bench.py: a gloo
 * broadcast); every rank then calls ljmd_comm_init, which joins the communicator with the
 * rank / n_ranks given to ljmd_create.  ljmd_allgather_positions enqueues ONE in-place
 * ncclAllGather of 3*P doubles per rank on the handle's stream -- ordered behind
 * ljmd_step_begin's kernels and ahead of ljmd_step_finish's, no host synchronisation.
 * With n_ranks = 1 it is a no-op and needs no communicator.
 */
#define LJMD_COMM_ID_BYTES 128
int ljmd_comm_unique_id(char *id_out /* [LJMD_COMM_ID_BYTES] */);
int ljmd_comm_init(ljmd_t *h, const char *id /* [LJMD_COMM_ID_BYTES] */);
int ljmd_allgather_positions(ljmd_t *h);
/* Ranks RCCL itself reports for this handle's communicator (ncclCommCount); 0 = no communicator.
 * bench.py prints it so that a multi-GPU line proves the collective ran over all ranks. */
int32_t ljmd_comm_size(const ljmd_t *h);
/*
 * Ownership migration of a multi-GPU run, on the devices.  A rank owns a fixed SET of particles, which in a liquid
 * diffuses out of the region it filled when it was dealt (about 4 sigma rms in 10 000 steps): the rank's 64-particle
 * tiles grow and the tile-pair test skips less (-9 % step rate over 10 000 steps at n = 65536 on 8 ranks).  A migration
 * deals all n particles out again BY POSITION: every rank packs ru, v, a and the particle ids of its slots, one all-gather
 * (80 n bytes over xGMI; the positions are in the exchange buffer already) brings everybody's to every rank, every rank
 * computes the same split of the n particles into G parts of exactly n / G (stable radix sorts on identical input:
 * identical result everywhere; x-slabs by default, near-cubic k-d blocks with LJMD_MIGRATE_DEAL=blocks -- same total work,
 * but only the translation-symmetric slabs give every rank the same share under the pair kernel's ownership rule), keeps
 * part `rank`, re-sorts it into tiles and joins the next position all-gather.  Between two MD steps only (no step half enqueued); pending step records and a snapshot in flight are
 * not affected.  No arithmetic of the path changes: the trajectory differs only by summation order.
 *   ljmd_migrate           everything, collectives included: a multi-device handle (ljmd_create_multi; also done
 *                          automatically every LJMD_MULTI_MIGRATE_EVERY steps, default 2000, and at ljmd_set_state), or a
 *                          rank engine with an RCCL communicator (every rank calls it at the same step); no-op for 1 rank
 *   ljmd_migrate_pack / _buffer / _deal   the phases around a caller-made exchange of the G blocks of the migration
 *                          buffer (block g: 10 P doubles at offset g * 10 P; host-staged fallback, tests); the caller then
 *                          also repeats the position exchange
 *   ljmd_particle_ids      ids[j], j < n / n_ranks: index, in the arrays given to the last ljmd_set_state, of the particle at
 *                          position j of this rank engine's arrays (ljmd_get_state, ljmd_snapshot_end); rank S + j until a
 *                          migration.  ljmd_set_accel / ljmd_set_unwrapped keep taking the GLOBAL arrays in that order.
 *                          (A multi-device handle keeps the caller's order itself: identity.)
 *   ljmd_multi_migrations  migrations done so far on this handle
 */
int ljmd_migrate(ljmd_t *h);
int ljmd_migrate_pack(ljmd_t *h);
void *ljmd_migrate_buffer(ljmd_t *h, int64_t *n_doubles_total, int64_t *own_offset_doubles, int64_t *own_count_doubles);
int ljmd_migrate_deal(ljmd_t *h);
int ljmd_particle_ids(ljmd_t *h, int32_t *ids);
int32_t ljmd_multi_migrations(const ljmd_t *h);
/* Copy on the handle's stream, then wait: kind 1 = host->device, 2 = device->host, 3 = device->device.
 * For callers that stage the exchange / force buffers themselves (host-staged fallback, tests). */
int ljmd_memcpy(ljmd_t *h, void *dst, const void *src, int64_t bytes, int32_t kind);
/* Blocks the host until everything enqueued on the handle's stream (and device) is done. */
int ljmd_synchronize(ljmd_t *h);
/* The HIP stream (hipStream_t) all of this handle's kernels are launched on. */
void *ljmd_stream(ljmd_t *h);
/* Phase 1: drift + wrap + half-kick + unwrapped update of the owned shard; the new
 * positions are written into the own block of the exchange buffer. */
int ljmd_step_begin(ljmd_t *h);
/*
 * Phase 2 (after the all-gather): pair forces of this rank's share of the pair matrix
 * against all n positions; with the Newton-3 kernel on n_ranks > 1 the library then sums
 * the partial accelerations across ranks with ONE ncclReduceScatter of 3*P doubles per rank
 * on the handle's stream; second half-kick; per-rank partial sums appended to the scalar ring.
 */
int ljmd_step_finish(ljmd_t *h);
/* Pair forces only (t = 0 evaluation) on the exchange buffer contents. */
int ljmd_forces_partial(ljmd_t *h);
/*
 * Test / integration hooks.  ljmd_step_forces runs only the pair kernel + slab reduction of
 * phase 2 (ljmd_step_finish / ljmd_forces_partial then continue from there).  ljmd_force_buffers
 * exposes the partial-acceleration buffer fpart ([n_ranks][3][P], block g = contributions to
 * rank g's particles) and the receive buffer frecv ([3][P]); with external != 0 the library
 * skips its own reduce-scatter and expects the caller to have written sum_ranks fpart[g] into
 * rank g's frecv before ljmd_step_finish (used to emulate several ranks on one GPU).
 */
int ljmd_step_forces(ljmd_t *h);
int ljmd_force_buffers(ljmd_t *h, int32_t external, void **fpart, int64_t *fpart_doubles,
                       void **frecv, int64_t *frecv_doubles);
/*
 * Copies out the raw per-rank partial records of the last `nsteps` finished phases,
 * LJMD_PARTIAL_STRIDE (8) doubles each: { sum r^-12, sum r^-6 over this rank's ordered
 * pairs, sum vx^2, sum vy^2, sum vz^2 over its particles, 0, 0, 0 }.  Resets the ring.
 */
int ljmd_read_partials(ljmd_t *h, int32_t nsteps, double *partial);
/* Host-side, deterministic: combines the n_ranks partial records of ONE step (rank
 * order) into epot, ekin, d_epot, dd_epot incl. prefactors and tail corrections. */
int ljmd_combine_scalars(const ljmd_t *h, const double *partials_by_rank, int32_t n_ranks,
                         double *epot, double *ekin, double *d_epot, double *dd_epot);

/* The reproducible mode's form of the two calls above: records of LJMD_EXACT_PARTIAL_WORDS int64 words (ljmd_read_partials
 * returns LJMD_ERR_STATE on such a handle), combined as integers before the single rounding of each scalar;
 * LJMD_ERR_RANGE when a record carries the range flag. */
int ljmd_read_partials_exact(ljmd_t *h, int32_t nsteps, int64_t *words);
int ljmd_combine_scalars_exact(const ljmd_t *h, const int64_t *words_by_rank, int32_t n_ranks,
                               double *epot, double *ekin, double *d_epot, double *dd_epot);

/*
 * The reference's switch `use_tail_corrections` (scripts/physics/lj_potential_energy.f90:36, a compile-time
 * parameter, .true. as shipped; :205-223): on = 0 leaves the three mean-field tail constants out of epot, d_epot and
 * dd_epot -- of every scalar this handle returns from now on (they are added on the host when the step records are
 * combined; forces never contain them).  ljmd_stateless_set_tail_corrections does the same for the cached engine behind
 * the stateless drop-ins ljmd_compute_lj_potential_energy / ljmd_verlet_step (process-wide, default on); the Fortran shim
 * modules pass their own `use_tail_corrections` parameter through it on every call.
 */
int ljmd_set_tail_corrections(ljmd_t *h, int32_t on);
void ljmd_stateless_set_tail_corrections(int32_t on);

/* ---- measurement --------------------------------------------------------- */

/*
 * Live HIP-event timing on the handle's own stream.  After ljmd_profile_enable(h, 1)
 * every step / force evaluation records events around its kernels; ljmd_profile_read
 * waits for the stream and returns averages per launch in milliseconds:
 *   ms_avg[0] pair-force kernel          ms_avg[1] geometry pre-pass (tile boxes + mask)
 *   ms_avg[2] drift/kick kernel (+ re-sort)   ms_avg[3] slab reduce + kick + finalize
 * *launches = number of launches averaged; the counters are reset.
 */
int ljmd_profile_enable(ljmd_t *h, int32_t on);
/* Name of the pair-force kernel the next force evaluation will launch (for profile matching). */
const char *ljmd_pair_kernel_name(const ljmd_t *h);
int ljmd_profile_read(ljmd_t *h, double *ms_avg /* [4] */, int32_t *launches);
/* Same, plus the minimum over the launches of each interval (ms_min[2] = the drift/kick kernel alone:
 * the steps that also re-sort are longer).  Either array may be NULL. */
int ljmd_profile_read_ex(ljmd_t *h, double *ms_avg /* [4] */, double *ms_min /* [4] */, int32_t *launches);
/* Per rank, with the two exchanges of a multi-GPU step: intervals 0..3 as above, ms[4] = the position
 * all-gather, ms[5] = the force reduce-scatter / all-to-all (HIP events on the stream that carries the collective,
 * from the moment this rank could start it: the wait for the slowest rank is part of it; 0 when the launches had no
 * exchange).  `rank` selects the rank engine of a multi-device handle (ljmd_create_multi); on an ordinary engine it
 * must be the engine's own rank.  Resets that rank's counters. */
int ljmd_profile_read_rank(ljmd_t *h, int32_t rank, double *ms_avg /* [6] */, double *ms_min /* [6] */,
                           int32_t *launches);
/* The same with the median over the launches of each interval: what tells a 1-2 % kernel change from the +-3 % a box
 * differs from the next by (bench.py: roofline.kernel_ms_min / kernel_ms_median).  Any array may be NULL. */
int ljmd_profile_read_stats(ljmd_t *h, int32_t rank, double *ms_avg /* [6] */, double *ms_min /* [6] */,
                            double *ms_median /* [6] */, int32_t *launches);

/*
 * g(r) of the resident system, accumulated where the positions live (ljmd_rdf_*): no snapshot leaves the device.
 *
 * Definition.  One snapshot adds to hist[nbins], for the positions resident now -- the wrapped r that ljmd_get_state
 * would return and ljmd_snapshot_begin would copy -- exactly the integers ljmd_rdf_histogram(n, x, y, z, L, nbins, rmax,
 * hist) adds for those positions: weight 2 per unordered pair with r < rmax, bin int(r / dr), dr = rmax / nbins, through
 * the same per-pair arithmetic with no contraction, over all particles (no subsampling).  The counts are integers, so
 * they depend on nothing else: not on the slot order or re-sort state, the tile walk, the number of ranks, ownership
 * migration, the precision mode, knobs or streams.
 * configure: 1 <= nbins <= LJMD_RDF_MAX_BINS, rmax finite and > 0 (values above L/2 are allowed, as in the stateless
 * call); allocates and zeroes the counts and the snapshot count; calling it again reconfigures and zeroes; nbins == 0
 * switches the feature off and frees it.  A failed guard returns LJMD_ERR_INVALID_ARG and leaves the earlier
 * configuration in place; a failed allocation LJMD_ERR_ALLOC with the feature off.  Works with or without a state.
 * ljmd_set_state, ljmd_set_accel, ljmd_set_unwrapped and ljmd_set_tail_corrections leave configuration and counts alone.
 * accumulate: one snapshot, stream-ordered on the engine's stream behind everything enqueued so far
 * (ljmd_enqueue_steps* included), no host wait; the snapshot count goes up by one.  LJMD_ERR_STATE before configure,
 * without a state, without valid accelerations, on a poisoned handle and between ljmd_step_begin and ljmd_step_finish.
 * r, ru, v, a, the step records and every later result stay bitwise what they are without the call: it reads the
 * exchange buffer and writes buffers of its own.
 * read: waits for the device; hist[nbins] and the snapshot count, either may be NULL; clears nothing.
 * reset: zeroes both.  read, reset and profile_read return LJMD_ERR_STATE before configure.
 * profile_read, for the most recent accumulate (zeros before the first): the (row tile, column tile) pairs of 64 x 64
 * particles its walk evaluated, the pairs it considered (evaluated + skipped because their bounding boxes are provably
 * farther apart than rmax), and the time of its two launches from HIP events; any pointer may be NULL; waits for the
 * device.
 * Ranks.  On a rank engine (ljmd_create with n_ranks > 1) a snapshot adds weight 1 for every ordered pair (i owned by
 * this rank, j any other particle of the system) and read returns this partial histogram: the partials of the ranks add
 * up to the definition above.  The rank's exchange buffer must hold everybody's current positions, which is the case
 * whenever the accelerations are valid and the caller has run the exchanges it is responsible for (after
 * ljmd_migrate_deal: the position exchange).  On a multi-device handle (ljmd_create_multi) accumulate runs on every
 * rank, read returns the sum, the snapshot count is the common one; profile_read returns the tile-pair counts summed
 * over the ranks and the longest of their times.
 */
#define LJMD_RDF_MAX_BINS 8192
int ljmd_rdf_configure(ljmd_t *h, int32_t nbins, double rmax);
int ljmd_rdf_accumulate(ljmd_t *h);
int ljmd_rdf_read(ljmd_t *h, uint64_t *hist, int64_t *n_snapshots);
int ljmd_rdf_reset(ljmd_t *h);
int ljmd_rdf_profile_read(ljmd_t *h, int64_t *tile_pairs_visited, int64_t *tile_pairs_total, double *kernel_ms);

/*
 * MSD(tau) and VACF(tau) of the resident system, time-origin averaged where ru and v live (ljmd_tcf_*): no snapshot
 * leaves the device.  One-rank engines only (ljmd_create with n_ranks = 1).
 *
 * Definition.  That of ljmd_batch_tcf_* below with B = 1 -- the terms, Q(t) = RNE(t 2^64), the range rule (a term that
 * is not finite or has |t| >= 2^40 enters as 0 and sets a sticky range word), signed 192-bit sums S[kind][l] per (kind,
 * lag), the lag-0 terms of an origin added when the next snapshot arrives, ring slot (s / origin_stride) % slots with
 * slots = max_lag / origin_stride + 1 <= LJMD_TCF_MAX_ORIGINS, count[l] kept on the host, msd[l] = fixed(S[0][l]) /
 * ((double)n * (double)count[l]) through ljmd_tcf_from_exact.  What differs:
 *   Snapshot: the resident ru and v of all n particles, as ljmd_get_state would return them now; numbered s = 0, 1, ...
 *   from the last configure, reset or ljmd_set_state.
 *   Identity: a term pairs values of the same particle, i.e. the same index of the arrays given to the last
 *   ljmd_set_state, whatever slot it occupies now.  The integers therefore depend on the snapshots alone: not on slot
 *   order, re-sort state or interval, tiling knobs, step form (generic, Newton-3, two-launch fused step), precision mode
 *   (given the same ru, v) or on how the kernels split the work.
 * configure: 1 <= max_lag <= LJMD_TCF_MAX_LAG, origin_stride >= 1 (and n <= 2^23); max_lag = 0 switches the feature off and frees
 * everything; otherwise allocates and zeroes; calling it again reconfigures and zeroes.  A failed guard returns
 * LJMD_ERR_INVALID_ARG and leaves the earlier configuration in place; a failed allocation LJMD_ERR_ALLOC with the
 * feature off, the message naming the buffer and its byte count.  Works with or without a state.  The origin ring is
 * slots x 6 x n_pad x 8 bytes, n_pad = n rounded up to 1024 -- 6.4 GB at n = 262 144 with 512 origins; the size is
 * computed in size_t.  On a rank engine (n_ranks > 1) or a multi-device handle (ljmd_create_multi) configure returns
 * LJMD_ERR_INVALID_ARG ("... n_ranks = <G>: ... needs a one-rank engine"), and the other five calls LJMD_ERR_STATE
 * ("not configured").
 * accumulate: the resident state is the next snapshot, stream-ordered on the engine's stream behind everything enqueued
 * so far (ljmd_enqueue_steps* included), no host wait.  Guards and their order are those of ljmd_rdf_accumulate:
 * LJMD_ERR_STATE before configure, without a state, without valid accelerations, on a poisoned handle and between
 * ljmd_step_begin and ljmd_step_finish.  It writes only buffers of its own: r, ru, v, a, the step records, the slot
 * permutation and every later result stay bitwise what they are without the call.
 * read / read_exact: wait for the device; msd[max_lag + 1], vacf[max_lag + 1] (read) or words[2][max_lag + 1][3]
 * (read_exact), counts[max_lag + 1], the number of snapshots since configure / reset -- any pointer may be NULL; they
 * clear nothing.  With the range word set they return LJMD_ERR_RANGE until ljmd_tcf_reset; the handle is not poisoned
 * and stepping is unaffected.
 * reset: zeroes the sums, counts, numbering and range word.
 * profile_read, for the most recent accumulate (zeros before the first): the HIP-event time of its launches and the
 * number of live origins it visited; either pointer may be NULL; waits for the device.
 * read, read_exact, reset and profile_read return LJMD_ERR_STATE before configure.
 * ljmd_set_state starts a new trajectory: the stored origins are dropped and the numbering restarts at 0, the sums and
 * counts stay, as for the batch.  ljmd_set_unwrapped, ljmd_set_accel, ljmd_set_tail_corrections, ljmd_rdf_* and
 * ljmd_migrate (a no-op on one rank) leave everything alone.
 */
#define LJMD_TCF_MAX_LAG 4096
#define LJMD_TCF_MAX_ORIGINS 512
int ljmd_tcf_configure(ljmd_t *h, int32_t max_lag, int32_t origin_stride);
int ljmd_tcf_accumulate(ljmd_t *h);
int ljmd_tcf_read(ljmd_t *h, double *msd, double *vacf, int64_t *counts, int64_t *n_snapshots);
int ljmd_tcf_read_exact(ljmd_t *h, int64_t *words /* [2][max_lag+1][3] */, int64_t *counts, int64_t *n_snapshots);
int ljmd_tcf_reset(ljmd_t *h);
int ljmd_tcf_profile_read(ljmd_t *h, double *kernel_ms, int32_t *origins_live);

/*
 * Van Hove self-correlation G_s(r, tau) = < delta(r - |ru_i(t0 + tau) - ru_i(t0)|) > of the resident system, the
 * distribution behind the MSD, time-origin averaged where ru lives (ljmd_vanhove_*): no snapshot leaves the device.
 * One-rank engines only (ljmd_create with n_ranks = 1).
 *
 * Definition.  Parameters max_lag, origin_stride, nbins, rmax; dr = rmax / nbins.  Snapshots, their numbering s, the
 * origin rule and the ring slot are those of ljmd_tcf_* above, word for word: a snapshot is stored as an origin when
 * s % origin_stride == 0, in ring slot (s / origin_stride) % slots with slots = max_lag / origin_stride + 1 <=
 * LJMD_VANHOVE_MAX_ORIGINS; an origin t0 contributes at 1 <= s - t0 <= max_lag; the lag-0 row of an origin is added
 * when the next snapshot arrives; count[l] is kept on the host; a term pairs a particle with itself by id, the index
 * in the arrays of the last ljmd_set_state.  A snapshot here is the resident ru only (numbered from the last
 * configure, reset or ljmd_set_state).  Per particle i, origin t0 and lag l, unfused and left to right:
 *   d = ru(t0 + l) - ru(t0) per axis ;  r2 = (dx*dx + dy*dy) + dz*dz     (the MSD term of ljmd_tcf_*, bit for bit)
 *   r4 = r2 * r2 ;  r = sqrt(r2) (correctly rounded) ;  bin = int(r / dr) exactly (the true quotient, truncated)
 *   H[l][bin] += 1 for bin < nbins, else H[l][nbins] += 1 (the overflow column); H is [max_lag + 1][nbins + 1] uint64
 *   S2[l] += Q(r2), S4[l] += Q(r4), Q(t) = RNE(t 2^64): signed 192-bit integers, three int64 limbs, least significant
 *   first (the layout of ljmd_tcf_read_exact)
 * Range: when r2 or r4 is not finite or |r4| >= 2^40 the particle counts in the overflow column, enters both sums as 0
 * and sets a sticky range word.  Invariants: every row of H sums to n count[l]; S2 equals ljmd_tcf_*'s S[MSD] for the
 * same snapshots and the same (max_lag, origin_stride), integer for integer.  The integers depend on the snapshots
 * alone: not on slot order, re-sort state or interval, tiling knobs, step form, precision mode (given the same ru) or
 * on how the kernels split the work (LJMD_VANHOVE_CHUNK, read at ljmd_create: live origins per slice of the grid).
 * r2[l] = fixed(S2[l]) / ((double)n * (double)count[l]) and r4[l] likewise, through ljmd_tcf_from_exact: one rounding,
 * one division, 0 where count[l] == 0.  The non-Gaussian parameter is alpha2 = 3 r4 / (5 r2^2) - 1.
 * configure: 1 <= max_lag <= LJMD_VANHOVE_MAX_LAG, origin_stride >= 1, 1 <= nbins <= LJMD_VANHOVE_MAX_BINS, rmax finite
 * and > 0 (rmax / nbins a normal number), n <= 2^23; max_lag = 0 switches the feature off and frees everything (the
 * other arguments are then ignored); otherwise allocates and zeroes; calling it again reconfigures and zeroes.  A
 * failed guard returns LJMD_ERR_INVALID_ARG and leaves the earlier configuration in place; a failed allocation
 * LJMD_ERR_ALLOC with the feature off, the message naming the buffer and its byte count.  Works with or without a
 * state.  The origin ring, the feature's own (not that of ljmd_tcf_*), is slots x 3 x n_pad x 8 bytes, n_pad = n rounded
 * up to 1024 -- 3.2 GB at n = 262 144 with 512 origins; every size is computed in size_t.  On a rank engine (n_ranks > 1)
 * or a multi-device handle (ljmd_create_multi) configure returns LJMD_ERR_INVALID_ARG ("... n_ranks = <G>: ... needs a
 * one-rank engine"), and the other five calls LJMD_ERR_STATE ("not configured").
 * accumulate: the resident ru is the next snapshot, stream-ordered on the engine's stream behind everything enqueued so
 * far (ljmd_enqueue_steps* included), no host wait.  Guards and their order are those of ljmd_rdf_accumulate.  It
 * writes only buffers of its own: r, ru, v, a, the step records, the slot permutation, the other observables and every
 * later result stay bitwise what they are without the call.
 * read / read_exact: wait for the device; hist[max_lag + 1][nbins + 1], r2[max_lag + 1], r4[max_lag + 1] (read) or
 * words[2][max_lag + 1][3], S2 then S4 (read_exact), counts[max_lag + 1], the number of snapshots since configure /
 * reset -- any pointer may be NULL; they clear nothing.  With the range word set they return LJMD_ERR_RANGE until
 * ljmd_vanhove_reset; the handle is not poisoned and stepping is unaffected.
 * reset: zeroes the histogram, sums, counts, numbering and range word.
 * profile_read, for the most recent accumulate (zeros before the first): the HIP-event time of its launches and the
 * number of live origins it visited; either pointer may be NULL; waits for the device.
 * read, read_exact, reset and profile_read return LJMD_ERR_STATE before configure.
 * ljmd_set_state starts a new trajectory: the stored origins are dropped and the numbering restarts at 0; histogram,
 * sums and counts stay.  The other setters, ljmd_rdf_*, ljmd_tcf_*, ljmd_stress_*, ljmd_heatflux_* and ljmd_migrate leave
 * everything alone.
 */
#define LJMD_VANHOVE_MAX_LAG 4096
#define LJMD_VANHOVE_MAX_ORIGINS 512
#define LJMD_VANHOVE_MAX_BINS 4096
int ljmd_vanhove_configure(ljmd_t *h, int32_t max_lag, int32_t origin_stride, int32_t nbins, double rmax);
int ljmd_vanhove_accumulate(ljmd_t *h);
int ljmd_vanhove_read(ljmd_t *h, uint64_t *hist /* [max_lag+1][nbins+1] */, double *r2 /* [max_lag+1] */,
                      double *r4 /* [max_lag+1] */, int64_t *counts, int64_t *n_snapshots);
int ljmd_vanhove_read_exact(ljmd_t *h, uint64_t *hist, int64_t *words /* [2][max_lag+1][3]: S2 then S4 */,
                            int64_t *counts, int64_t *n_snapshots);
int ljmd_vanhove_reset(ljmd_t *h);
int ljmd_vanhove_profile_read(ljmd_t *h, double *kernel_ms, int32_t *origins_live);

/*
 * Pressure tensor of the resident system, one snapshot per call, recorded where r and v live (ljmd_stress_*): no
 * snapshot leaves the device.  One-rank engines, rank engines and multi-device handles; n <= 2^23.
 *
 * Definition.  Components c in the order xx, yy, zz, xy, xz, yz.  One snapshot is 12 signed 192-bit integers, K[6]
 * then S[6], each three int64 limbs, least significant first (the layout of ljmd_tcf_read_exact).
 *   Kinetic part: for every particle the terms vx*vx, vy*vy, vz*vz, vx*vy, vx*vz, vy*vz of the resident velocities, each
 *   entering K[c] as Q(t) = RNE(t 2^64).
 *   Virial part, over the ORDERED pairs i != j of the wrapped positions resident now, the arithmetic of the
 *   reproducible mode's pair kernel, unfused, left to right:
 *     d0 = x_i - x_j ; d = d0 - L * round(d0 * invL) (half away from zero) per axis ; r2 = dx*dx + dy*dy + dz*dz ;
 *     if r2 < rc2 (strict): u = 1.0 / r2 ; u3 = u*u*u ; u6 = u3*u3 ; mdu = 2.0*u6 - u3 ; fx = mdu*dx*u, fy, fz likewise;
 *     terms fx*dx, fy*dy, fz*dz, fx*dy, fx*dz, fy*dz, each entering S[c] as Q(t).
 *   Under i <-> j every d and f changes sign exactly, so an unordered pair may be evaluated once and added twice: the
 *   integer is the same.
 *   Range: a pair is out of range when any of fx, fy, fz, u6 or of its six products is not finite or has |t| >= 2^40;
 *   all six of its terms then enter as 0 and a sticky word is set.  The same holds for a particle's six velocity
 *   products.  An arithmetic flag: nothing wraps, nothing faults.
 *   Doubles: p[c] = (R(K[c]) + 12.0 * R(S[c])) / V with V = (L*L)*L and R(x) = RNE(x) 2^-64, ONE rounding of the integer
 *   -- the host-only ljmd_stress_from_exact(words[12][3], L, out[6]).  No tail correction: ljmd_set_tail_corrections
 *   does not apply, and the isotropic tail term is the caller's to add to the diagonal.  12 (S_xx + S_yy + S_zz) is
 *   -(d_epot without tail) up to per-term rounding; K_xx + K_yy + K_zz is 2 ekin.
 * The integers depend on the particle set alone: not on slot order, re-sorts, tiling, ranks, ownership migration,
 * precision mode or knobs.
 * configure: 1 <= max_snapshots <= LJMD_STRESS_MAX_SNAPSHOTS and n <= 2^23; allocates and zeroes the series on the
 * device (288 bytes per snapshot); calling it again reconfigures and zeroes; 0 switches the feature off and frees it.
 * A failed guard returns LJMD_ERR_INVALID_ARG and leaves the earlier configuration in place; a failed allocation
 * LJMD_ERR_ALLOC with the feature off.  Works with or without a state.  ljmd_set_state, the other setters, ljmd_rdf_*,
 * ljmd_tcf_* and ljmd_migrate leave configuration and series alone.
 * accumulate: appends one snapshot, stream-ordered on the engine's stream behind everything enqueued so far
 * (ljmd_enqueue_steps* included), no host wait.  Guards and their order are those of ljmd_rdf_accumulate:
 * LJMD_ERR_STATE before configure, without a state, without valid accelerations, on a poisoned handle and between
 * ljmd_step_begin and ljmd_step_finish; then LJMD_ERR_STATE when the series is full, before anything is launched.  It
 * reads the exchange buffer and the velocities and writes only buffers of its own: r, ru, v, a, the step records and
 * every later result stay bitwise what they are without the call.
 * read_exact / read: wait for the device; words[n][12][3] (read_exact) or p[n][6] (read) for the n snapshots taken
 * since configure / reset, and n -- any pointer may be NULL; they clear nothing.  While the sticky word is set they
 * return LJMD_ERR_RANGE, until ljmd_stress_reset; the handle is not poisoned and stepping is unaffected.
 * reset: empties the series and clears the sticky word.
 * profile_read, for the most recent accumulate (zeros before the first): the (row tile, column tile) pairs of 64 x 64
 * particles its walk evaluated, the pairs it considered (evaluated + skipped because their bounding boxes are provably
 * farther apart than rc), and the time of its launches from HIP events; any pointer may be NULL; waits for the device.
 * read_exact, read, reset and profile_read return LJMD_ERR_STATE before configure.
 * Ranks.  On a rank engine (ljmd_create with n_ranks > 1) a snapshot sums the ordered pairs (i owned by this rank, j
 * any other particle of the system) and the velocity products of the own particles, and read_exact returns this
 * partial: the partials of the ranks add up, as integers, to the definition above.  read is refused there
 * (LJMD_ERR_STATE: add the words, then ljmd_stress_from_exact).  The rank's exchange buffer must hold everybody's
 * current positions, which is the case whenever the accelerations are valid and the caller has run the exchanges it
 * is responsible for (after ljmd_migrate_deal: the position exchange).  On a multi-device handle (ljmd_create_multi)
 * accumulate runs on every rank, read_exact / read add the ranks' words in 192 bits on the host, profile_read returns
 * the tile-pair counts summed over the ranks and the longest of their times.
 */
#define LJMD_STRESS_MAX_SNAPSHOTS 262144
int ljmd_stress_configure(ljmd_t *h, int32_t max_snapshots);
int ljmd_stress_accumulate(ljmd_t *h);
int ljmd_stress_read_exact(ljmd_t *h, int64_t *words /* [n][12][3] */, int64_t *n_snapshots);
int ljmd_stress_read(ljmd_t *h, double *p /* [n][6] */, int64_t *n_snapshots);
int ljmd_stress_reset(ljmd_t *h);
int ljmd_stress_profile_read(ljmd_t *h, int64_t *tile_pairs_visited, int64_t *tile_pairs_total, double *kernel_ms);
int ljmd_stress_from_exact(const int64_t *words /* [12][3] */, double box_length, double *out6);

/*
 * Heat flux of the resident system, one snapshot per call, recorded where r and v live (ljmd_heatflux_*): no snapshot
 * leaves the device.  Its autocorrelation is the Green-Kubo integrand of the thermal conductivity.  One-rank engines
 * only (ljmd_create with n_ranks = 1); n <= 2^23.
 *
 * Definition.  One snapshot is 9 signed 192-bit integers, E[3] then P[3] then C[3] with axes x, y, z, each three int64
 * limbs, least significant first (the layout of ljmd_stress_read_exact): 216 bytes.  All arithmetic is unfused, left
 * to right, and a term t enters its integer as Q(t) = RNE(t 2^64).
 *   Convective part: for every particle k2 = vx*vx + vy*vy + vz*vz of the resident velocities and the terms k2*vx,
 *   k2*vy, k2*vz, entering E[a].
 *   Pair parts, over the ORDERED pairs i != j of the wrapped positions resident now; the minimum image and the pair
 *   arithmetic are those of ljmd_stress_* above, word for word:
 *     d0 = x_i - x_j ; d = d0 - L * round(d0 * invL) (half away from zero) per axis ; r2 = dx*dx + dy*dy + dz*dz ;
 *     if r2 < rc2 (strict): u = 1.0 / r2 ; u3 = u*u*u ; u6 = u3*u3 ; mdu = 2.0*u6 - u3 ; fx = mdu*dx*u, fy, fz likewise;
 *     wx = vx_i + vx_j, wy, wz likewise ; phi = u6 - u3 ; g = fx*wx + fy*wy + fz*wz ;
 *     potential terms phi*wx, phi*wy, phi*wz entering P[a]; collisional terms g*dx, g*dy, g*dz entering C[a].
 *   Under i <-> j w, r2 and phi keep their bits, every d, every f and g change sign exactly: all six terms are the same
 *   from both sides, so an unordered pair may be evaluated once and added twice -- the integer is the same.
 *   Range: a pair is out of range when any of fx, fy, fz, u6, wx, wy, wz, g or of its six terms is not finite or has
 *   |t| >= 2^40; all six of its terms then enter as 0 and a sticky word is set.  The same holds for a particle's k2 and
 *   its three terms.  An arithmetic flag: nothing wraps, nothing faults.
 *   Doubles: j[a] = (0.5 * R(E[a]) + R(P[a]) + 6.0 * R(C[a])) / V with V = (L*L)*L and R(x) = RNE(x) 2^-64, ONE rounding
 *   of each integer; parts[p][a] holds the three summands, each divided by V, in the order convective, potential,
 *   collisional -- the host-only ljmd_heatflux_from_exact(words[9][3], L, j[3], parts[3][3] or NULL).
 *   Where the factors come from.  The Irving-Kirkwood flux of a pair potential is
 *     J V = sum_i e_i v_i + 1/2 sum_{i != j} (F_ij . v_i) r_ij ,   e_i = 1/2 v_i^2 + 1/2 sum_{j != i} phi_ij ,
 *   with phi_ij = 4 (u6 - u3), F_ij = 24 f (the force on i from j) and r_ij = d.  The kinetic energies give 1/2 E.  The
 *   potential energies give 1/2 sum_{i != j} 4 phi v_i; phi is symmetric, so v_i may be replaced by (v_i + v_j) / 2:
 *   1/4 * 4 = 1 times P.  In the last sum (F_ij . v_i) r_ij and (F_ji . v_j) r_ji = (F_ij . v_j) r_ij are the two
 *   orders of one pair, so v_i may be replaced by (v_i + v_j) / 2 as well: 1/4 * 24 = 6 times C.  No tail correction:
 *   ljmd_set_tail_corrections does not apply.  No enthalpy term: a one-component system at zero total momentum needs
 *   none.
 * The integers depend on the particle set alone: not on slot order, re-sorts, tiling, precision mode or knobs.
 * configure: 1 <= max_snapshots <= LJMD_HEATFLUX_MAX_SNAPSHOTS and n <= 2^23; allocates and zeroes the series on the
 * device; calling it again reconfigures and zeroes; 0 switches the feature off and frees it.  A failed guard returns
 * LJMD_ERR_INVALID_ARG and leaves the earlier configuration in place; a failed allocation LJMD_ERR_ALLOC with the
 * feature off.  Works with or without a state.  On a rank engine (n_ranks > 1) or a multi-device handle
 * (ljmd_create_multi) configure with max_snapshots > 0 returns LJMD_ERR_INVALID_ARG ("... n_ranks = <G>: a pair term
 * needs the velocities of both particles and a rank holds only its own ..."), and the other five calls LJMD_ERR_STATE
 * ("not configured").  ljmd_set_state, the other setters, ljmd_rdf_*, ljmd_tcf_*, ljmd_stress_* and ljmd_migrate leave
 * configuration and series alone, and it leaves theirs alone.
 * accumulate: appends one snapshot, stream-ordered on the engine's stream behind everything enqueued so far
 * (ljmd_enqueue_steps* included), no host wait.  Guards and their order are those of ljmd_stress_accumulate:
 * LJMD_ERR_STATE before configure, without a state, without valid accelerations, on a poisoned handle and between
 * ljmd_step_begin and ljmd_step_finish; then LJMD_ERR_STATE when the series is full, before anything is launched.  It
 * reads the exchange buffer and the velocities and writes only buffers of its own: r, ru, v, a, the step records, the
 * other three observables and every later result stay bitwise what they are without the call.
 * read_exact / read: wait for the device; words[n][9][3] (read_exact) or j[n][3] and parts[n][3][3] (read) for the n
 * snapshots taken since configure / reset, and n -- any pointer may be NULL; they clear nothing.  While the sticky word
 * is set they return LJMD_ERR_RANGE, until ljmd_heatflux_reset; the handle is not poisoned and stepping is unaffected.
 * reset: empties the series and clears the sticky word.
 * profile_read, for the most recent accumulate (zeros before the first): the tile pairs its walk evaluated, those it
 * considered, and the time of its launches from HIP events, as ljmd_stress_profile_read; any pointer may be NULL.
 * read_exact, read, reset and profile_read return LJMD_ERR_STATE before configure.
 */
#define LJMD_HEATFLUX_MAX_SNAPSHOTS 262144
int ljmd_heatflux_configure(ljmd_t *h, int32_t max_snapshots);
int ljmd_heatflux_accumulate(ljmd_t *h);
int ljmd_heatflux_read_exact(ljmd_t *h, int64_t *words /* [n][9][3] */, int64_t *n_snapshots);
int ljmd_heatflux_read(ljmd_t *h, double *j /* [n][3] */, double *parts /* [n][3][3], may be NULL */, int64_t *n_snapshots);
int ljmd_heatflux_reset(ljmd_t *h);
int ljmd_heatflux_profile_read(ljmd_t *h, int64_t *tile_pairs_visited, int64_t *tile_pairs_total, double *kernel_ms);
int ljmd_heatflux_from_exact(const int64_t *words /* [9][3] */, double box_length, double *j3, double *parts9 /* may be NULL */);

/*
 * Collective density modes of the resident system, rho_k(t) = sum_j exp(i k . r_j(t)) with k = (2 pi / L) (n_x, n_y, n_z)
 * for a list of integer triples n, one snapshot per call, recorded where r lives (ljmd_rhok_*): no snapshot leaves the
 * device.  S(k) = <|rho_k|^2> / N and the coherent intermediate scattering function F(k, tau) = <Re rho_k(t0 + tau)
 * rho_k*(t0)> / N follow from this one series (analysis.static_structure_factor, analysis.intermediate_scattering).
 * One-rank engines only (ljmd_create with n_ranks = 1); n <= 2^23.  Sign convention: rho_k = sum (cos k.r, + sin k.r).
 *
 * Definition.  One snapshot is, per mode of the list in list order, two signed 192-bit integers Re then Im, each three
 * int64 limbs, least significant first (the layout of ljmd_stress_read_exact): 48 bytes per mode.  Everything is fp64
 * with separate roundings, no fused multiply-add anywhere; rint is round-half-even.  Per particle and mode, with x, y, z
 * the positions that ljmd_get_state returns as r (the exchange buffer) and n the mode's triple converted to double:
 *     t_a  = x_a / L ;  t_a = t_a - rint(t_a)                 (a = x, y, z; IEEE division; the subtraction is exact)
 *     phi  = (n_x*t_x + n_y*t_y) + n_z*t_z                     (each product and each sum rounded once)
 *     f    = phi - rint(phi)                                   (exact, |f| <= 1/2)
 *     q    = rint(4*f) ;  g = f - 0.25*q                       (exact, |g| <= 1/8; q in -2 .. 2)
 *     th   = g * 0x1.921fb54442d18p+2 ;  zz = th*th
 *     ps   = S15 ; ps = ps*zz + S13 ; ... ; ps = ps*zz + S3 ;  s = th + th*(zz*ps)
 *     pc   = C16 ; pc = pc*zz + C14 ; ... ; pc = pc*zz + C2 ;  c = 1.0 + zz*pc
 *     (q & 3) = 0: (C, S) = (c, s)    1: (-s, c)    2: (-c, -s)    3: (s, -c)
 *     Re[m] += Q(C) ;  Im[m] += Q(S)                           with Q(t) = RNE(t 2^64)
 *   The coefficients are the correctly rounded doubles of (-1)^j / (2j+1)! and (-1)^j / (2j)!:
 *     S3 = -0x1.5555555555555p-3    S5 = 0x1.1111111111111p-7     S7 = -0x1.a01a01a01a01ap-13   S9 = 0x1.71de3a556c734p-19
 *     S11 = -0x1.ae64567f544e4p-26  S13 = 0x1.6124613a86d09p-33   S15 = -0x1.ae7f3e733b81fp-41
 *     C2 = -0x1p-1                  C4 = 0x1.5555555555555p-5     C6 = -0x1.6c16c16c16c17p-10   C8 = 0x1.a01a01a01a01ap-16
 *     C10 = -0x1.27e4fb7789f5cp-22  C12 = 0x1.1eed8eff8d898p-29   C14 = -0x1.93974a8c07c9dp-37  C16 = 0x1.ae7f3e733b81fp-45
 *   Given f, C and S are within 1.4 2^-53 of cos 2 pi f and sin 2 pi f; the whole term is within
 *   2 pi 2^-53 sum_a |n_a| (|x_a| / L + 1.5) + 2^-51 of the true cos / sin of k . r.
 *   Range: a term is out of range when C or S is not finite, which happens with a coordinate or an L that is not; it
 *   then enters as two zeros and sets a sticky word.  An arithmetic flag: nothing wraps, nothing faults.
 *   Padding slots of the engine's layout are not particles: they add nothing and set no flag.
 *   Symmetry: the arithmetic is odd / even symmetric, so mode -n has the same Re words and exactly negated Im words;
 *   mode (0, 0, 0) has Re = n 2^64 and Im = 0.
 *   Doubles: rho[m] = (R(Re[m]), R(Im[m])) with R(x) = RNE(x) 2^-64, ONE rounding of each integer.
 * The integers depend on the positions and the mode list alone: not on slot order, re-sorts, grid shape, precision mode
 * or knobs; a mode's words do not depend on the rest of the list.
 * select_modes: pure host code without a handle, the list the drivers use.  The triples of the half-space (n_x > 0, or
 * n_x = 0 and n_y > 0, or n_x = n_y = 0 and n_z > 0) with 1 <= |n|^2 <= n2_max <= LJMD_RHOK_MAX_INDEX^2, grouped by |n|^2
 * ascending, within a shell lexicographic in (n_x, n_y, n_z); a shell with count > per_shell members keeps the members
 * at indices floor(j count / per_shell), j = 0 .. per_shell - 1.  *n_modes receives the number of modes; with capacity
 * too small the call returns LJMD_ERR_INVALID_ARG with the needed count in *n_modes (modes may then be NULL for
 * capacity = 0).
 * configure: 1 <= n_modes <= LJMD_RHOK_MAX_MODES triples of |n_a| <= LJMD_RHOK_MAX_INDEX -- (0, 0, 0), negatives and
 * duplicates included -- 1 <= max_snapshots <= LJMD_RHOK_MAX_SNAPSHOTS, max_snapshots * n_modes <= LJMD_RHOK_MAX_ENTRIES
 * and n <= 2^23; copies the list to the device, allocates and zeroes the series there; calling it again reconfigures
 * and zeroes; max_snapshots = 0 switches the feature off and frees everything, whatever the other arguments.  A failed
 * guard returns LJMD_ERR_INVALID_ARG and leaves the earlier configuration in place; a failed allocation LJMD_ERR_ALLOC
 * with the feature off.  Works with or without a state.  On a rank engine (n_ranks > 1) or a multi-device handle
 * (ljmd_create_multi) configure with max_snapshots > 0 returns LJMD_ERR_INVALID_ARG ("... n_ranks = <G>: a rank holds
 * only its own particles ..."), and the other calls LJMD_ERR_STATE ("not configured").  The setters, ljmd_migrate and
 * the other five observables leave configuration and series alone, and it leaves theirs alone.
 * accumulate: appends one snapshot, stream-ordered on the engine's stream behind everything enqueued so far
 * (ljmd_enqueue_steps* included), no host wait.  It needs a state but no accelerations: LJMD_ERR_STATE before
 * configure, without a state, on a poisoned handle and between ljmd_step_begin and ljmd_step_finish; then
 * LJMD_ERR_STATE when the series is full, before anything is launched.  It reads the exchange buffer and the slot
 * permutation and writes only buffers of its own: r, ru, v, a, the step records, the other five observables and every
 * later result stay bitwise what they are without the call.  Switched off it launches nothing, and no existing kernel
 * knows of it.
 * read_exact / read: wait for the device; words[n][n_modes][2][3] (read_exact) or rho[n][n_modes][2] (read) for the n
 * snapshots taken since configure / reset, and n -- any pointer may be NULL; they clear nothing.  While the sticky word
 * is set they return LJMD_ERR_RANGE, until ljmd_rhok_reset; the handle is not poisoned and stepping is unaffected.
 * reset: empties the series and clears the sticky word.
 * profile_read, for the most recent accumulate (zero before the first): the time of its launches from HIP events; the
 * pointer may be NULL; waits for the device.
 * read_exact, read, reset and profile_read return LJMD_ERR_STATE before configure.
 */
#define LJMD_RHOK_MAX_MODES 4096
#define LJMD_RHOK_MAX_INDEX 1023            /* |n_a| of a mode */
#define LJMD_RHOK_MAX_SNAPSHOTS 262144
#define LJMD_RHOK_MAX_ENTRIES (1 << 24)     /* max_snapshots * n_modes: 805 MB of series */
int ljmd_rhok_select_modes(int32_t n2_max, int32_t per_shell, int32_t capacity, int32_t *modes /* [capacity][3] */, int32_t *n_modes);
int ljmd_rhok_configure(ljmd_t *h, int32_t n_modes, const int32_t *modes /* [n_modes][3] */, int32_t max_snapshots);
int ljmd_rhok_accumulate(ljmd_t *h);
int ljmd_rhok_read_exact(ljmd_t *h, int64_t *words /* [n][n_modes][2][3]: Re then Im */, int64_t *n_snapshots);
int ljmd_rhok_read(ljmd_t *h, double *rho /* [n][n_modes][2] */, int64_t *n_snapshots);
int ljmd_rhok_reset(ljmd_t *h);
int ljmd_rhok_profile_read(ljmd_t *h, double *kernel_ms);

/*
 * Collective current modes of the resident system, j_k(t) = sum_j v_j(t) exp(i k . r_j(t)) with k = (2 pi / L) n for a
 * list of integer triples n, one snapshot per call, recorded where r and v live (ljmd_current_*): no snapshot leaves the
 * device.  The projections of j_k along and across k give the longitudinal and transverse current correlation functions
 * C_L(k, tau) and C_T(k, tau) and the wave-vector dependent shear viscosity eta(k) on the host
 * (analysis.current_correlations, analysis.current_equal_time, analysis.transverse_viscosity).  One-rank engines only
 * (ljmd_create with n_ranks = 1); n <= 2^23.  Independent of ljmd_rhok_*: either, both or neither may be configured.
 *
 * Definition.  One snapshot is, per mode of the list in list order, six signed 192-bit integers in the order x Re, x Im,
 * y Re, y Im, z Re, z Im, each three int64 limbs, least significant first: words[snapshot][n_modes][3][2][3], 144 bytes
 * per mode.  Everything is fp64 with separate roundings, no fused multiply-add anywhere.  Per live particle and mode, with
 * x, y, z and v_x, v_y, v_z the r and v that ljmd_get_state returns:
 *     (C, S)      exactly the (C, S) of ljmd_rhok_* above for these positions and this mode
 *     P_a = v_a * C ;  R_a = v_a * S                            (a = x, y, z; one product each, rounded once)
 *     Re_a[m] += Q(P_a) ;  Im_a[m] += Q(R_a)                     with Q(t) = RNE(t 2^64), |Q| < 2^104
 *   Range: the (particle, mode) term is out of range when C or S is not finite, or when any of the six products is not
 *   finite or has magnitude >= 2^40; it then enters all six sums as zero and sets a sticky word.  An arithmetic flag:
 *   nothing wraps, nothing faults.  Padding slots of the engine's layout are not particles: they add nothing and set no
 *   flag.
 *   Bound: with B the bound of the density modes' term above, P_a and R_a, as the numbers Q(.) 2^-64, are within
 *   |v_a| (B + 2^-53 (1 + B)) + 2^-65 of the true v_a cos k.r and v_a sin k.r: |v_a| times B, one product rounding,
 *   one quantisation.
 *   Consequences, each exact: (1) mode -n has the same Re words and exactly negated Im words; (2) mode (0, 0, 0) has
 *   Re_a = sum_j Q(v_a) and Im_a = 0, the total momentum with no padding slot counted; (3) with every velocity equal to
 *   (1, -1, 2) the x words are the words of ljmd_rhok_* for the same positions and modes and the y words their negation
 *   (a product by +-1 is exact and Q is odd); the z words are the sums of Q(2 C) and Q(2 S), exactly twice the words of
 *   ljmd_rhok_* where every term is 0 or has magnitude >= 2^-12 -- t 2^64 is then an integer and Q(2 t) = 2 Q(t) -- and
 *   within one unit per smaller term of twice them otherwise (RNE(2 x) = 2 RNE(x) only for x within 1/4 of an integer);
 *   (4) the velocities are those ljmd_get_state returns as v, paired with its r.
 *   Doubles: j[m][a] = (R(Re_a[m]), R(Im_a[m])) with R(x) = RNE(x) 2^-64, ONE rounding of each integer.
 * The integers depend on the positions, the velocities and the mode list alone: not on slot order, re-sorts, grid shape,
 * precision mode or knobs; a mode's words do not depend on the rest of the list.
 * The mode list obeys the rules of ljmd_rhok_configure (LJMD_RHOK_MAX_MODES, LJMD_RHOK_MAX_INDEX; (0, 0, 0), negatives
 * and duplicates included), and ljmd_rhok_select_modes gives the drivers' shell-wise list.
 * configure: 1 <= max_snapshots <= LJMD_CURRENT_MAX_SNAPSHOTS, max_snapshots * n_modes <= LJMD_CURRENT_MAX_ENTRIES and
 * n <= 2^23; copies the list to the device, allocates and zeroes the series there; calling it again reconfigures and
 * zeroes; max_snapshots = 0 switches the feature off and frees everything, whatever the other arguments.  A failed guard
 * returns LJMD_ERR_INVALID_ARG and leaves the earlier configuration in place; a failed allocation LJMD_ERR_ALLOC with the
 * feature off.  Works with or without a state.  On a rank engine (n_ranks > 1) or a multi-device handle configure with
 * max_snapshots > 0 returns LJMD_ERR_INVALID_ARG ("... n_ranks = <G>: a rank holds only its own particles ..."), and the
 * other calls LJMD_ERR_STATE ("not configured").  The setters, ljmd_migrate and the other six observables leave
 * configuration and series alone, and it leaves theirs alone.
 * accumulate: appends one snapshot, stream-ordered on the engine's stream behind everything enqueued so far, no host
 * wait.  It needs a state but no accelerations: LJMD_ERR_STATE before configure, without a state, on a poisoned handle
 * and between ljmd_step_begin and ljmd_step_finish; then LJMD_ERR_STATE when the series is full, before anything is
 * launched.  It reads the exchange buffer, the velocities and the slot permutation and writes only buffers of its own:
 * r, ru, v, a, the step records, the other six observables and every later result stay bitwise what they are without
 * the call.  Switched off it launches nothing, and no existing kernel knows of it.
 * read_exact / read: wait for the device; words[n][n_modes][3][2][3] (read_exact) or j[n][n_modes][3][2] (read) for the
 * n snapshots taken since configure / reset, and n -- any pointer may be NULL; they clear nothing.  While the sticky word
 * is set they return LJMD_ERR_RANGE, until ljmd_current_reset; the handle is not poisoned and stepping is unaffected.
 * reset: empties the series and clears the sticky word.
 * profile_read, for the most recent accumulate (zero before the first): the time of its launches from HIP events; the
 * pointer may be NULL; waits for the device.
 * read_exact, read, reset and profile_read return LJMD_ERR_STATE before configure.
 */
#define LJMD_CURRENT_MAX_SNAPSHOTS 262144
#define LJMD_CURRENT_MAX_ENTRIES (1 << 22)   /* max_snapshots * n_modes: 604 MB of series at 144 bytes per entry */
int ljmd_current_configure(ljmd_t *h, int32_t n_modes, const int32_t *modes /* [n_modes][3] */, int32_t max_snapshots);
int ljmd_current_accumulate(ljmd_t *h);
int ljmd_current_read_exact(ljmd_t *h, int64_t *words /* [n][n_modes][3][2][3] */, int64_t *n_snapshots);
int ljmd_current_read(ljmd_t *h, double *j /* [n][n_modes][3][2] */, int64_t *n_snapshots);
int ljmd_current_reset(ljmd_t *h);
int ljmd_current_profile_read(ljmd_t *h, double *kernel_ms);

/* ---- batch engine: many independent small systems on one device ------------------------------------------------
 *
 * One ljmd_batch_t holds B replicas on one device -- the ensemble runs of the reference's run-many framework
 * (scripts/run_many_md_simuations/run_many_md.f90), or a sweep over state points -- and steps all of them with one
 * kernel, one workgroup per replica, many steps per launch.  ljmd_batch_create gives every replica the same
 * (n, L, dt, rc); ljmd_batch_create_per_replica gives replica b its own (n_b, L_b, dt_b, rc_b).  Each replica is
 * exactly the physics of an ljmd_t.
 *
 * Layout: per-particle arrays are fp64 with offsets[B] = sum n_b elements, the replicas concatenated in replica order
 * (element (b, i) at offsets[b] + i; ljmd_batch_offsets; for ljmd_batch_create offsets[b] = b*n, replica-major);
 * per-replica scalars have B elements; the scalars of ljmd_batch_steps are [nsteps / sample_every][B], sample-major.
 * Every other ljmd_batch_* call works the same on both kinds of handle.
 *
 * Arithmetic, per replica, is the single engine's fast path (ljmd_kernels.hip):
 *   drift + wrap + half-kick + unwrapped update: drift_kick_kernel's expressions in the same order, no contraction,
 *     so with the same a(t) the positions after one step are bit-exact;
 *   pair term: pair_fast in full-matrix gather form -- every ordered pair (i, j != i), minimum image
 *     fma(-L, rint(d/L), d), r^2 = fma(dz, dz, fma(dy, dy, dx*dx)), strict r^2 < rc^2, 1/r^2 by v_rcp_f64 + one
 *     Halley step -- the energy sums halved afterwards;
 *   kick: a = 24 f, v += a dt/2, three separate sums of v^2; scalars combined on the host as for an ljmd_t
 *     (tail constants included while ljmd_batch_set_tail_corrections is on, the default).
 * Tolerances against the reference are those of the single engine.
 *
 * Determinism: every floating-point sum of a replica runs in an order fixed by its n alone, with no floating-point
 * atomics, so a replica's results are bitwise equal run to run and independent of B, of its slot in the batch and
 * of what the other replicas hold: with its own (n, L, dt, rc) a replica gives the bits of a one-replica
 * ljmd_batch_create handle of the same replica, whatever the other replicas' parameters, their order, the grouping
 * into launches or the streams.  The energy sums are evaluated only on sampled steps; r, ru, v, a are bitwise the
 * same for every sample_every, and with no outputs at all.
 *
 * Reproducible batches (ljmd_batch_set_precision with LJMD_PRECISION_FP64_REPRODUCIBLE): per replica, exactly the
 * definition of LJMD_PRECISION_FP64_REPRODUCIBLE above -- the pair terms of that definition over every ordered pair,
 * each entering a 128-bit integer sum as Q(t); a = 24 R(sum) with one rounding; S12, S6, Kx, Ky, Kz as exact 192-bit
 * integers per replica (the ordered-pair sums halved as integers), ONE rounding per scalar, then the tail constants;
 * ljmd_batch_kinetic_energy = 0.5 ((Kx + Ky) + Kz) of that definition; the integrator is the fp64 mode's.  A
 * replica's results are then a function of its particle set alone: bitwise equal to tests/reproducible_model.py and to
 * an ljmd_t of the same mode, and on top of the invariances above independent of the order of its particles (permuted
 * input gives the permuted state and the same scalars).  Range: every term of every step, sampled or not, must be
 * finite with |t| < 2^40; otherwise the term enters as 0, the replica's sticky flag is set, and the call
 * (ljmd_batch_steps, ljmd_batch_compute_forces or ljmd_batch_kinetic_energy) fails with LJMD_ERR_RANGE, its message
 * naming the lowest such replica ("replica <b>"); the handle is poisoned until ljmd_batch_set_state, which also clears
 * the flags.  Launches hold fewer steps than in the fp64 mode (a pair costs several times as much).
 *
 * Limits: n <= LJMD_BATCH_MAX_N -- one replica's positions live in one CU's LDS for a whole launch, 24 n bytes
 * <= 96 KiB; the creators take LJMD_PRECISION_FP64 only (the mode of a new handle; the reproducible mode is selected
 * afterwards with ljmd_batch_set_precision, no other mode exists for batches); rc <= (1 - 1e-9) L/2 and, at
 * ljmd_batch_set_state, every replica's coordinates finite and spanning < 2.4 L per axis (each replica against its
 * own L) (the fast path's preconditions (b) and (a)): there is no generic-kernel fallback in this mode, so such input
 * fails with LJMD_ERR_INVALID_ARG.  All guards run before the device probe; without a device ljmd_batch_create
 * returns LJMD_ERR_NO_DEVICE.
 *
 * g(r) (ljmd_batch_rdf_*): the pair-distance histogram of every replica's resident wrapped positions, accumulated on
 * the device into [B][nbins] 64-bit counts -- per replica exactly the integers ljmd_rdf_histogram adds for that
 * snapshot (weight 2 per unordered pair with r < rmax_b, bin int(r / dr_b), dr_b = rmax_b / nbins; all particles, no
 * subsampling), so the counts are independent of B, slot, launch grouping, streams and precision mode.
 * ljmd_batch_rdf_accumulate adds one snapshot; with every > 0 ljmd_batch_steps adds the positions after steps every,
 * 2 every, ... of each call by itself, leaving r, ru, v, a and the sampled scalars bitwise what they are without it.
 *
 * Sequence: ljmd_batch_steps before ljmd_batch_set_state, or before valid accelerations (ljmd_batch_compute_forces
 * or ljmd_batch_set_accel), returns LJMD_ERR_STATE.  A launch that fails poisons the handle (LJMD_ERR_STATE) until
 * ljmd_batch_set_state.  A handle is not thread-safe; one handle is one device.
 */
#define LJMD_BATCH_MAX_N 4096
typedef struct ljmd_batch ljmd_batch_t;

int ljmd_batch_create(ljmd_batch_t **out, int32_t n_replicas, int32_t n, double box_length, double dt, double rc,
                      int32_t precision_mode, int32_t device);
/* B replicas, replica b with its own n[b], box_length[b], dt[b], rc[b] (arrays of n_replicas elements).  Every replica
 * passes the guards of ljmd_batch_create; the sum of n must be < 2^31.  Failures before the device probe return
 * LJMD_ERR_INVALID_ARG, the message starting "ljmd_batch_create_per_replica: replica <b>:" when one replica is at fault. */
int ljmd_batch_create_per_replica(ljmd_batch_t **out, int32_t n_replicas, const int32_t *n,
                                  const double *box_length, const double *dt, const double *rc,
                                  int32_t precision_mode, int32_t device);
/* offsets[B + 1]: replica b's particles are elements [offsets[b], offsets[b+1]) of every per-particle array. */
int ljmd_batch_offsets(const ljmd_batch_t *h, int64_t *offsets);
void ljmd_batch_destroy(ljmd_batch_t *h);
/* Text of the most recent error on this handle (h == NULL: the thread's last failed ljmd_batch_create). */
const char *ljmd_batch_last_error(const ljmd_batch_t *h);
/* As ljmd_set_state for every replica: a = 0, ru = r.  All six arrays required. */
int ljmd_batch_set_state(ljmd_batch_t *h, const double *rx, const double *ry, const double *rz,
                         const double *vx, const double *vy, const double *vz);
/* NULL = keep that component. */
int ljmd_batch_set_accel(ljmd_batch_t *h, const double *ax, const double *ay, const double *az);
int ljmd_batch_set_unwrapped(ljmd_batch_t *h, const double *ux, const double *uy, const double *uz);
/* Any NULL = skipped. */
int ljmd_batch_get_state(ljmd_batch_t *h, double *rx, double *ry, double *rz,
                         double *ux, double *uy, double *uz,
                         double *vx, double *vy, double *vz,
                         double *ax, double *ay, double *az);
/* Forces of every replica (overwrites a); epot, d_epot, dd_epot: [B] each or NULL. */
int ljmd_batch_compute_forces(ljmd_batch_t *h, double *epot, double *d_epot, double *dd_epot);
/* ekin[B]: 0.5 sum (vx^2 + vy^2 + vz^2), the fused sum of ljmd_kinetic_energy. */
int ljmd_batch_kinetic_energy(ljmd_batch_t *h, double *ekin);
/*
 * nsteps x { verlet_step ; unwrapped update } on every replica, no host synchronisation inside; returns once the
 * results are on the host.  The scalars of steps sample_every, 2 sample_every, ... go to [nsteps / sample_every][B]
 * arrays (each NULL or such an array); nsteps % sample_every == 0 and nsteps / sample_every <=
 * LJMD_MAX_PENDING_STEPS.  With all four arrays NULL no step is sampled and sample_every is not used.
 */
int ljmd_batch_steps(ljmd_batch_t *h, int32_t nsteps, int32_t sample_every,
                     double *epot, double *ekin, double *d_epot, double *dd_epot);
/* As ljmd_set_tail_corrections. */
int ljmd_batch_set_tail_corrections(ljmd_batch_t *h, int32_t on);
/* LJMD_PRECISION_FP64 (the default of a new handle) or LJMD_PRECISION_FP64_REPRODUCIBLE; anything else:
 * LJMD_ERR_INVALID_ARG and the handle keeps its mode.  The resident accelerations belong to the old mode:
 * the handle then needs ljmd_batch_set_state again (LJMD_ERR_STATE from steps / compute_forces until then).
 * Setting the mode the handle already has changes nothing.  Works on both kinds of handle. */
int ljmd_batch_set_precision(ljmd_batch_t *h, int32_t precision_mode);
/* Kernel time (HIP events, ms) and launch count of the last ljmd_batch_steps call; either pointer may be NULL.
 * Both include the g(r), MSD / VACF, pressure tensor, heat flux and van Hove launches of that call
 * (ljmd_batch_rdf_configure / ljmd_batch_tcf_configure / ljmd_batch_stress_configure / ljmd_batch_heatflux_configure /
 * ljmd_batch_vanhove_configure with every > 0).
 * Replicas of different kernel classes (n <= 128, 512, 1024, 2048, 4096) run as separate groups of launches, by
 * default each on a stream of its own (LJMD_BATCH_GROUP_STREAMS=0: one after another on the handle's stream); the
 * kernel time is then the span from the first group's first launch to the last group's end, not a sum over groups,
 * and the launch count is the total over all groups. */
int ljmd_batch_profile_read(const ljmd_batch_t *h, double *kernel_ms, int32_t *launches);
/*
 * g(r) histograms on the device.  configure: nbins bins per replica (1 <= nbins <= 8192; 0 switches the feature off
 * and frees the histogram), rmax[B] (each finite and > 0) or NULL = 0.5 L_b, every >= 0; allocates and zeroes the
 * [B][nbins] counts and the snapshot count; calling it again reconfigures and zeroes.  A failed guard returns
 * LJMD_ERR_INVALID_ARG ("ljmd_batch_rdf_configure: replica <b>: ..." where one replica is at fault) and leaves the
 * earlier configuration in place.  every > 0: ljmd_batch_steps accumulates the positions after steps every,
 * 2 every, ... of each call (independent of sample_every); its nsteps must then be a multiple of every
 * (LJMD_ERR_INVALID_ARG before anything is launched).  ljmd_batch_set_precision and ljmd_batch_set_state leave the
 * configuration and the counts alone.  If a reproducible ljmd_batch_steps call fails with LJMD_ERR_RANGE, the counts
 * accumulated in that call are unspecified until ljmd_batch_rdf_reset.
 * accumulate: adds the histogram of the positions resident now, for every replica, stream-ordered (no host wait); the
 * snapshot count goes up by one.  LJMD_ERR_STATE before configure, before ljmd_batch_set_state or on a poisoned handle.
 * read: waits for the device, copies hist[B][nbins] (or NULL) and the snapshot count (or NULL); clears nothing.
 * reset: zeroes both.  read and reset return LJMD_ERR_STATE before configure.
 */
int ljmd_batch_rdf_configure(ljmd_batch_t *h, int32_t nbins, const double *rmax, int32_t every);
int ljmd_batch_rdf_accumulate(ljmd_batch_t *h);
int ljmd_batch_rdf_read(ljmd_batch_t *h, uint64_t *hist, int64_t *n_snapshots);
int ljmd_batch_rdf_reset(ljmd_batch_t *h);
/*
 * MSD(tau) and VACF(tau), time-origin averaged, on the device (ljmd_batch_tcf_*) -- compute_msd_tau_timeorig /
 * compute_vacf_tau_timeorig of the reference (scripts/md_one_run_analysis.py:404-489) for every replica, as exact
 * integers before their normalisation.
 *
 * Definition.  Snapshots of a handle are numbered s = 0, 1, 2, ... from the last configure, reset or
 * ljmd_batch_set_state; a snapshot is the resident ru and v of every replica at that moment.  1 <= max_lag <=
 * LJMD_BATCH_TCF_MAX_LAG, origin_stride >= 1, max_lag / origin_stride + 1 <= LJMD_BATCH_TCF_MAX_ORIGINS.  Per replica b,
 * particle i, origin t0 and lag l, the reference's numpy expressions with no contraction:
 *   MSD  term: d = ru(t0 + l) - ru(t0) per axis, t = (dx*dx + dy*dy) + dz*dz
 *   VACF term: t = (vx(t0 + l)*vx(t0) + vy(t0 + l)*vy(t0)) + vz(t0 + l)*vz(t0)
 * Every term enters an exact signed integer sum as Q(t) = RNE(t 2^64).  Device state per replica: S[kind][l], kind 0 =
 * MSD, 1 = VACF, l = 0 .. max_lag, each a signed 192-bit integer of three little-endian 64-bit limbs; the host keeps
 * count[l], the same for all replicas.  When snapshot s arrives:
 *   1. for every stored origin t0 with t0 % origin_stride == 0 and 1 <= s - t0 <= max_lag:
 *      S[kind][s - t0] += sum_i Q(term_i), count[s - t0] += 1; if s - t0 == 1 also the lag-0 term of that origin:
 *      S[kind][0] += sum_i Q(term_i(t0, t0)), count[0] += 1 (the reference does not use the last snapshot as an origin;
 *      deferring lag 0 to the next snapshot reproduces that for any stopping point);
 *   2. if s % origin_stride == 0, snapshot s is stored as an origin, in ring slot (s / origin_stride) % slots, slots =
 *      max_lag / origin_stride + 1.
 * Result: msd[b][l] = fixed(S[0][l]) / ((double)n_b * (double)count[l]), fixed = ONE correctly rounded conversion of the
 * integer times 2^-64; vacf from S[1] likewise; 0 where count[l] == 0.  This equals the reference's functions on the same
 * snapshots to rounding (<= 1e-13 max|value|); the integers themselves are independent of B, slot, launch grouping,
 * streams, precision mode and the order of the particles.
 * Range: a term that is not finite or has |t| >= 2^40 enters as 0 and sets a sticky per-replica word in device memory
 * (an arithmetic flag: nothing wraps, nothing faults); read / read_exact then fail with LJMD_ERR_RANGE, the message
 * naming the lowest such replica ("replica <b>"), until ljmd_batch_tcf_reset.  Stepping is not affected and the handle
 * is not poisoned.  n <= 4096 terms below 2^104 fit 128 bits per (snapshot, origin); 192 bits hold any number of origins.
 *
 * configure: max_lag = 0 switches the feature off and frees everything; otherwise allocates and zeroes S, the range
 * words and the origin ring (slots x 6 planes of offsets[B] doubles); calling it again reconfigures and zeroes.  A
 * failed guard returns LJMD_ERR_INVALID_ARG and leaves the earlier configuration in place; a failed allocation
 * LJMD_ERR_ALLOC with the feature off.  every > 0: ljmd_batch_steps takes the snapshots after steps every, 2 every, ...
 * of each call; its nsteps must then be a multiple of every (LJMD_ERR_INVALID_ARG before anything is launched).  With
 * g(r) configured with an every too, a launch ends at the multiples of either.  r, ru, v, a and the sampled scalars
 * stay bitwise what they are without the feature; ljmd_batch_profile_read counts the new launches and their time.
 * accumulate: the resident state is the next snapshot, stream-ordered (no host wait).  LJMD_ERR_STATE before
 * configure, before ljmd_batch_set_state or on a poisoned handle.
 * read: waits for the device; msd[B][max_lag + 1], vacf[B][max_lag + 1], counts[max_lag + 1], the number of snapshots
 * taken since configure / reset -- any pointer may be NULL; clears nothing.  read_exact: words[B][2][max_lag + 1][3]
 * instead of the two quotients.  Both return LJMD_ERR_STATE before configure.
 * reset: zeroes the sums, counts, snapshot numbering and range words.
 * ljmd_batch_set_state starts a new trajectory: the stored origins are dropped and the numbering restarts at 0, the
 * sums and counts are kept, so several trajectories run one after another on one handle average together.
 * ljmd_batch_set_precision, ljmd_batch_set_unwrapped and ljmd_batch_set_accel leave everything alone.  If a call that
 * takes snapshots fails half-way (a poisoned handle), sums and counts are unspecified until ljmd_batch_tcf_reset.
 * ljmd_tcf_from_exact: one sum of 3 limbs -> fixed(S) / ((double)n * (double)count), 0 for count == 0; host code only.
 */
#define LJMD_BATCH_TCF_MAX_LAG 4096
#define LJMD_BATCH_TCF_MAX_ORIGINS 512
int ljmd_batch_tcf_configure(ljmd_batch_t *h, int32_t max_lag, int32_t origin_stride, int32_t every);
int ljmd_batch_tcf_accumulate(ljmd_batch_t *h);
int ljmd_batch_tcf_read(ljmd_batch_t *h, double *msd, double *vacf, int64_t *counts, int64_t *n_snapshots);
int ljmd_batch_tcf_read_exact(ljmd_batch_t *h, int64_t *words, int64_t *counts, int64_t *n_snapshots);
int ljmd_batch_tcf_reset(ljmd_batch_t *h);
int ljmd_tcf_from_exact(const int64_t *words, int32_t n, int64_t count, double *out);
/*
 * Pressure tensor of every replica, a series of snapshots on the device (ljmd_batch_stress_*).
 *
 * Definition.  Per replica b one snapshot is exactly the 12 signed 192-bit integers K[6], S[6] of ljmd_stress_* above,
 * for that replica's own n_b, L_b, rc_b and its resident wrapped r and v: the components, the per-pair arithmetic,
 * Q(t) = RNE(t 2^64), the range rule and the limb layout are those of that comment.  The integers depend on the replica's
 * particle set alone: not on B, its slot, the other replicas, launch grouping, group streams, precision mode or the
 * order of the particles.  The series is sample-major like the scalars of ljmd_batch_steps: words[snapshot][B][12][3],
 * p[snapshot][B][6] with p = ljmd_stress_from_exact(words, L_b, .) per (snapshot, replica).
 * configure: 0 <= max_snapshots <= LJMD_BATCH_STRESS_MAX_SNAPSHOTS, every >= 0; max_snapshots = 0 switches the feature
 * off and frees it; otherwise allocates and zeroes 288 B max_snapshots bytes and a sticky range word per replica;
 * calling it again reconfigures and zeroes.  A failed guard returns LJMD_ERR_INVALID_ARG and leaves the earlier
 * configuration in place; a failed allocation LJMD_ERR_ALLOC with the feature off.  ljmd_batch_set_state,
 * ljmd_batch_set_precision, ljmd_batch_set_accel, ljmd_batch_set_unwrapped, ljmd_batch_set_tail_corrections, the
 * ljmd_batch_rdf_* / ljmd_batch_tcf_* calls and ljmd_batch_prepare leave configuration and series alone; the warm-up of
 * ljmd_batch_prepare takes no snapshot.
 * accumulate: appends one snapshot of every replica, stream-ordered (no host wait).  LJMD_ERR_STATE before configure,
 * before ljmd_batch_set_state, on a poisoned handle, and then when the series is full, before anything is launched.
 * every > 0: ljmd_batch_steps appends the state after steps every, 2 every, ... of each call; its nsteps must then be a
 * multiple of every (LJMD_ERR_INVALID_ARG), and a call whose snapshots do not all fit the series is refused with
 * LJMD_ERR_STATE, both before anything is launched.  r, ru, v, a and the sampled scalars stay bitwise what they are
 * without the feature; ljmd_batch_profile_read counts the new launches and their time.  A call that fails half-way (a
 * poisoned handle) leaves the snapshot count where it was.
 * read_exact / read: wait for the device; the n snapshots taken since configure / reset, and n -- any pointer may be
 * NULL; they clear nothing, and a poisoned handle may still be read.  While any replica's sticky word is set they return
 * LJMD_ERR_RANGE, the message naming the lowest such replica ("replica <b>"), until ljmd_batch_stress_reset; the handle
 * is not poisoned and stepping goes on.  reset: empties the series and clears the words.  accumulate, read_exact, read
 * and reset return LJMD_ERR_STATE before configure.
 */
#define LJMD_BATCH_STRESS_MAX_SNAPSHOTS 262144
int ljmd_batch_stress_configure(ljmd_batch_t *h, int32_t max_snapshots, int32_t every);
int ljmd_batch_stress_accumulate(ljmd_batch_t *h);
int ljmd_batch_stress_read_exact(ljmd_batch_t *h, int64_t *words /* [n][B][12][3] */, int64_t *n_snapshots);
int ljmd_batch_stress_read(ljmd_batch_t *h, double *p /* [n][B][6] */, int64_t *n_snapshots);
int ljmd_batch_stress_reset(ljmd_batch_t *h);
/*
 * Heat flux of every replica, a series of snapshots on the device (ljmd_batch_heatflux_*): the ensemble whose averaged
 * autocorrelation is the Green-Kubo integrand of the thermal conductivity.
 *
 * Definition.  Per replica b one snapshot is exactly the 9 signed 192-bit integers E[3], P[3], C[3] of ljmd_heatflux_*
 * above, for that replica's own n_b, L_b, rc_b and its resident wrapped r and v: the per-pair and per-particle
 * arithmetic, Q(t) = RNE(t 2^64), the range rule and the limb layout are those of that comment; 216 bytes.  The integers
 * depend on the replica's particle set alone: not on B, its slot, the other replicas, launch grouping, group streams,
 * precision mode or the order of the particles.  The series is sample-major like the scalars of ljmd_batch_steps:
 * words[snapshot][B][9][3], j[snapshot][B][3] and parts[snapshot][B][3][3] with (j, parts) =
 * ljmd_heatflux_from_exact(words, L_b, ., .) per (snapshot, replica).
 * configure: 0 <= max_snapshots <= LJMD_BATCH_HEATFLUX_MAX_SNAPSHOTS, every >= 0; max_snapshots = 0 switches the feature
 * off and frees it; otherwise allocates and zeroes 216 B max_snapshots bytes and a sticky range word per replica;
 * calling it again reconfigures and zeroes.  A failed guard returns LJMD_ERR_INVALID_ARG and leaves the earlier
 * configuration in place; a failed allocation LJMD_ERR_ALLOC with the feature off.  ljmd_batch_set_state,
 * ljmd_batch_set_precision, ljmd_batch_set_accel, ljmd_batch_set_unwrapped, ljmd_batch_set_tail_corrections, the
 * ljmd_batch_rdf_* / ljmd_batch_tcf_* / ljmd_batch_stress_* calls and ljmd_batch_prepare leave configuration and series
 * alone, and it leaves theirs alone; the warm-up of ljmd_batch_prepare takes no snapshot.
 * accumulate: appends one snapshot of every replica, stream-ordered (no host wait).  LJMD_ERR_STATE before configure,
 * before ljmd_batch_set_state, on a poisoned handle, and then when the series is full, before anything is launched.  It
 * reads r and v and writes only its own two buffers.
 * every > 0: ljmd_batch_steps appends the state after steps every, 2 every, ... of each call; its nsteps must then be a
 * multiple of every (LJMD_ERR_INVALID_ARG), and a call whose snapshots do not all fit the series is refused with
 * LJMD_ERR_STATE, both before anything is launched.  r, ru, v, a, the sampled scalars and the other three observables
 * stay bitwise what they are without the feature; ljmd_batch_profile_read counts the new launches and their time.  A
 * call that fails half-way (a poisoned handle) leaves the snapshot count where it was.
 * read_exact / read: wait for the device; the n snapshots taken since configure / reset, and n -- any pointer may be
 * NULL; they clear nothing, and a poisoned handle may still be read.  While any replica's sticky word is set they return
 * LJMD_ERR_RANGE, the message naming the lowest such replica ("replica <b>"), until ljmd_batch_heatflux_reset; the
 * handle is not poisoned and stepping goes on.  read_exact has then filled `words` all the same (an out-of-range pair or
 * particle entered as zeros; the other replicas' rows are whole) and left n_snapshots alone; read has written nothing.  reset: empties the series and clears the words.  accumulate, read_exact,
 * read and reset return LJMD_ERR_STATE before configure.
 */
#define LJMD_BATCH_HEATFLUX_MAX_SNAPSHOTS 262144
int ljmd_batch_heatflux_configure(ljmd_batch_t *h, int32_t max_snapshots, int32_t every);
int ljmd_batch_heatflux_accumulate(ljmd_batch_t *h);
int ljmd_batch_heatflux_read_exact(ljmd_batch_t *h, int64_t *words /* [n][B][9][3] */, int64_t *n_snapshots);
int ljmd_batch_heatflux_read(ljmd_batch_t *h, double *j /* [n][B][3] */, double *parts /* [n][B][3][3], may be NULL */, int64_t *n_snapshots);
int ljmd_batch_heatflux_reset(ljmd_batch_t *h);
/*
 * Van Hove self-correlation G_s(r, tau) of every replica, time-origin averaged, on the device (ljmd_batch_vanhove_*):
 * per replica, integer for integer, what ljmd_vanhove_* above is for B = 1.
 *
 * Definition.  Snapshots, their numbering s, the origin rule, the ring slot (s / origin_stride) % slots with slots =
 * max_lag / origin_stride + 1 <= LJMD_BATCH_VANHOVE_MAX_ORIGINS, the lag-0 row added when the next snapshot arrives and
 * count[l] on the host, the same for all replicas, are those of ljmd_batch_tcf_* above; a snapshot here is the resident
 * ru of every replica only, and the ring is the feature's own.  dr_b = rmax[b] / nbins.  Per replica b, particle i,
 * origin t0 and lag l, unfused and left to right:
 *   d = ru(t0 + l) - ru(t0) per axis ;  r2 = (dx*dx + dy*dy) + dz*dz     (the MSD term of ljmd_batch_tcf_*, bit for bit)
 *   r4 = r2 * r2 ;  r = sqrt(r2) (correctly rounded) ;  bin = int(r / dr_b) exactly (the true quotient, truncated)
 *   H[b][l][min(bin, nbins)] += 1 (column nbins is the overflow column); H is [B][max_lag + 1][nbins + 1] uint64
 *   S2[b][l] += Q(r2), S4[b][l] += Q(r4), Q(t) = RNE(t 2^64): signed 192-bit integers of three int64 limbs, least
 *   significant first
 * Range: when r2 or r4 is not finite or r4 >= 2^40 the particle counts in the overflow column, enters both sums as 0
 * and sets the replica's sticky range word (an arithmetic flag: nothing wraps, nothing faults, and no float-to-int
 * conversion sees such a value).  Invariants: every row H[b][l][.] sums to n_b count[l]; S2 equals the MSD words of
 * ljmd_batch_tcf_* configured with the same (max_lag, origin_stride) on the same handle, word for word.  The integers do
 * not depend on B, the replica's slot, the other replicas, launch grouping, group streams, precision mode (given the same
 * ru) or the order of the particles.  r2[b][l] = ljmd_tcf_from_exact(S2[b][l], n_b, count[l]) and r4[b][l] likewise: one
 * rounding, one division, 0 where count[l] == 0.  The non-Gaussian parameter is alpha2 = 3 r4 / (5 r2^2) - 1.
 * configure: the guards of ljmd_batch_tcf_configure in their order (max_lag in 0..LJMD_BATCH_VANHOVE_MAX_LAG, every >= 0,
 * origin_stride >= 1, the origin count), then 1 <= nbins <= LJMD_BATCH_VANHOVE_MAX_BINS, rmax not NULL, every rmax[b]
 * finite and > 0 with rmax[b] / nbins a normal number ("replica <b>").  max_lag = 0 switches the feature off and frees
 * everything (the arguments after it but `every` are then ignored); otherwise allocates and zeroes H, the sums, the
 * range words, dr_b and 1 / dr_b, and the origin ring (slots x 3 planes of offsets[B] doubles), every size computed in
 * size_t; calling it again reconfigures and zeroes.  A failed guard returns LJMD_ERR_INVALID_ARG and leaves the earlier
 * configuration in place; a failed allocation LJMD_ERR_ALLOC with the feature off, the message naming the buffer and its
 * byte count.  every > 0: ljmd_batch_steps takes the snapshots after steps every, 2 every, ... of each call; its nsteps
 * must then be a multiple of every (LJMD_ERR_INVALID_ARG before anything is launched); with other accumulators' every
 * set, a launch ends at the multiples of any of them, and the van Hove launch of a group is the last of a step.  r, ru,
 * v, a, the sampled scalars and the other four observables stay bitwise what they are without the feature;
 * ljmd_batch_profile_read counts the new launches and their time.  Off: no launch, no allocation, nothing else changes.
 * accumulate: the resident ru is the next snapshot, stream-ordered (no host wait).  LJMD_ERR_STATE before configure,
 * before ljmd_batch_set_state or on a poisoned handle.
 * read / read_exact: wait for the device; hist[B][max_lag + 1][nbins + 1], r2[B][max_lag + 1], r4[B][max_lag + 1] (read)
 * or words[B][2][max_lag + 1][3], S2 then S4 (read_exact), counts[max_lag + 1], the number of snapshots since configure /
 * reset -- any pointer may be NULL; they clear nothing, and a poisoned handle may still be read.  While any replica's
 * range word is set they fill the arrays all the same and then return LJMD_ERR_RANGE, the message naming the lowest such
 * replica ("replica <b>"), until ljmd_batch_vanhove_reset; the handle is not poisoned and stepping goes on.
 * reset: zeroes the histogram, sums, counts, snapshot numbering and range words.  read, read_exact and reset return
 * LJMD_ERR_STATE before configure.
 * ljmd_batch_set_state and ljmd_batch_prepare start a new trajectory: the stored origins are dropped and the numbering
 * restarts at 0; histogram, sums and counts stay.  The other setters and the other observables' calls leave everything
 * alone.  If a call that takes snapshots fails half-way (a poisoned handle), histogram, sums and counts are unspecified
 * until ljmd_batch_vanhove_reset.
 */
#define LJMD_BATCH_VANHOVE_MAX_LAG 4096
#define LJMD_BATCH_VANHOVE_MAX_ORIGINS 512
#define LJMD_BATCH_VANHOVE_MAX_BINS 1024
int ljmd_batch_vanhove_configure(ljmd_batch_t *h, int32_t max_lag, int32_t origin_stride, int32_t nbins,
                                 const double *rmax /* [B] */, int32_t every);
int ljmd_batch_vanhove_accumulate(ljmd_batch_t *h);
int ljmd_batch_vanhove_read(ljmd_batch_t *h, uint64_t *hist /* [B][max_lag+1][nbins+1] */,
                            double *r2 /* [B][max_lag+1] */, double *r4 /* [B][max_lag+1] */,
                            int64_t *counts /* [max_lag+1] */, int64_t *n_snapshots);
int ljmd_batch_vanhove_read_exact(ljmd_batch_t *h, uint64_t *hist, int64_t *words /* [B][2][max_lag+1][3]: S2 then S4 */,
                                  int64_t *counts, int64_t *n_snapshots);
int ljmd_batch_vanhove_reset(ljmd_batch_t *h);
/*
 * Collective density modes rho_k of every replica, a series of snapshots on the device (ljmd_batch_rhok_*): per replica,
 * integer for integer, what ljmd_rhok_* above records for one system -- the ensemble whose averaged S(k) and F(k, tau)
 * have an error bar (analysis.static_structure_factor_ensemble, analysis.intermediate_scattering_ensemble).
 *
 * Definition.  One list of modes is shared by the handle.  Per replica b one snapshot is, per mode of the list in list
 * order, exactly the two signed 192-bit integers Re then Im of ljmd_rhok_* above, for that replica's own n_b and L_b and
 * its resident wrapped r (what ljmd_batch_get_state returns as r): the arithmetic of a term, Q(t) = RNE(t 2^64), the
 * range rule, the symmetries and the limb layout are those of that comment; 48 bytes per mode.  The integers depend on
 * the replica's particle set and the mode alone: not on B, the replica's slot, the other replicas, launch grouping, group
 * streams, precision mode, the order of the particles or the rest of the list.  The series is sample-major like the
 * scalars of ljmd_batch_steps: words[snapshot][B][n_modes][2][3] and rho[snapshot][B][n_modes][2], rho = (R(Re), R(Im))
 * with R(x) = RNE(x) 2^-64, the one rounding of ljmd_rhok_read.
 * configure: 0 <= max_snapshots <= LJMD_BATCH_RHOK_MAX_SNAPSHOTS, every >= 0; max_snapshots = 0 switches the feature off
 * and frees it, whatever the mode arguments; otherwise the mode rules of ljmd_rhok_configure (1 <= n_modes <=
 * LJMD_RHOK_MAX_MODES triples of |n_a| <= LJMD_RHOK_MAX_INDEX, (0, 0, 0), negatives and duplicates included; the list
 * of ljmd_rhok_select_modes is the drivers') and max_snapshots * B * n_modes <= LJMD_BATCH_RHOK_MAX_ENTRIES; copies the
 * list to the device, allocates and zeroes 48 B n_modes max_snapshots bytes and a sticky range word per replica; calling
 * it again reconfigures and zeroes.  A failed guard returns LJMD_ERR_INVALID_ARG and leaves the earlier configuration in
 * place; a failed allocation LJMD_ERR_ALLOC with the feature off.  ljmd_batch_set_state, the other setters, the other
 * five observables' calls and ljmd_batch_prepare leave configuration and series alone, and it leaves theirs alone; the
 * warm-up of ljmd_batch_prepare takes no snapshot.
 * accumulate: appends one snapshot of every replica, stream-ordered (no host wait).  LJMD_ERR_STATE before configure,
 * before ljmd_batch_set_state, on a poisoned handle, and then when the series is full, before anything is launched.  It
 * needs no accelerations, reads r and writes only its own buffers.
 * every > 0: ljmd_batch_steps appends the state after steps every, 2 every, ... of each call; its nsteps must then be a
 * multiple of every (LJMD_ERR_INVALID_ARG), and a call whose snapshots do not all fit the series is refused with
 * LJMD_ERR_STATE, both before anything is launched; the density modes launch of a group, one per snapshot, is the last of
 * a step.  r, ru, v, a, the sampled scalars and the other five observables stay bitwise what they are without the
 * feature; ljmd_batch_profile_read counts the new launches and their time.  A call that fails half-way (a poisoned
 * handle) leaves the snapshot count where it was.  Off: no launch, no allocation, nothing else changes.
 * read_exact / read: wait for the device; the n snapshots taken since configure / reset, and n -- any pointer may be
 * NULL; they clear nothing, and a poisoned handle may still be read.  While any replica's sticky word is set they return
 * LJMD_ERR_RANGE, the message naming the lowest such replica ("replica <b>"), until ljmd_batch_rhok_reset; the handle is
 * not poisoned and stepping goes on.  read_exact has then filled `words` all the same (a term that was not finite
 * entered as zeros; the other replicas' rows are whole) and left n_snapshots alone; read has written nothing.  reset:
 * empties the series and clears the words.
 * profile_read, for the most recent ljmd_batch_rhok_accumulate (zero before the first): the time of its launches from HIP
 * events; the pointer may be NULL; waits for the device.
 * accumulate, read_exact, read, reset and profile_read return LJMD_ERR_STATE before configure.
 */
#define LJMD_BATCH_RHOK_MAX_SNAPSHOTS 262144
#define LJMD_BATCH_RHOK_MAX_ENTRIES (1 << 24)   /* max_snapshots * B * n_modes: 805 MB of series */
int ljmd_batch_rhok_configure(ljmd_batch_t *h, int32_t n_modes, const int32_t *modes /* [n_modes][3] */, int32_t max_snapshots,
                              int32_t every);
int ljmd_batch_rhok_accumulate(ljmd_batch_t *h);
int ljmd_batch_rhok_read_exact(ljmd_batch_t *h, int64_t *words /* [n][B][n_modes][2][3]: Re then Im */, int64_t *n_snapshots);
int ljmd_batch_rhok_read(ljmd_batch_t *h, double *rho /* [n][B][n_modes][2] */, int64_t *n_snapshots);
int ljmd_batch_rhok_reset(ljmd_batch_t *h);
int ljmd_batch_rhok_profile_read(ljmd_batch_t *h, double *kernel_ms);

/*
 * Independent initial configurations on the device (ljmd_batch_prepare): per replica b, with n = n_b, L = L_b and k the
 * integer with 4 k^3 = n, the steps of the reference's initial-configuration program
 * (scripts/md_initial_config_program.f90:58-121), without a round trip of the state through the host.  seeds[B] and
 * target_total_energy[B] are required; epot0[B] and ekin0[B] may be NULL.
 *   a. FCC lattice in the reference's particle order and expressions: cells ix > iy > iz, basis (0,0,0), (0,1/2,1/2),
 *      (1/2,0,1/2), (1/2,1/2,0); a = L / dble(k), x0 = dble(ix) * a, offsets x0 + 0.5 * a, no fused multiply-add.  ru <- r.
 *   b. Velocities from the reference's random_uniform as its first call with seed -|seeds[b]| initialises it: 3 n
 *      draws, particle i takes draws 3 i, 3 i + 1, 3 i + 2 for vx, vy, vz, v = draw - 0.5.  The generator's state is an
 *      integer m < 4 10^6 and a draw is double(m) * (1.0 / 4.0e6), the rounded reciprocal.  The stream depends on
 *      | 1618033 - |seed| | mod 4 10^6 alone: seeds s and -s, and seeds s and 3236066 - s, give the same stream.  Equal
 *      seeds in different replicas are allowed.
 *   c. Centre of mass per axis: v_cm = R(sum_i Q(v_i)) / dble(n), v_i <- v_i - v_cm, with Q(t) = rint(t 2^64) and R the
 *      one correctly rounded conversion of the exact integer sum, as in the reproducible mode -- in BOTH precision
 *      modes, so that the result depends on no summation order.
 *   d. epot0 = what ljmd_batch_compute_forces returns for this state (the handle's precision mode and tail-correction
 *      setting), ekin0 = what ljmd_batch_kinetic_energy returns for it; scale = sqrt((target - epot0) / ekin0) in IEEE
 *      doubles on the host; v <- v * scale on the device, one rounding each.  The accelerations of the force call stay
 *      valid (the positions did not change).
 *   e. warmup_steps velocity-Verlet steps as ljmd_batch_steps takes them, nothing sampled and no g(r), MSD, VACF,
 *      pressure tensor or heat flux snapshot taken whatever `every` is configured to; then ru <- r again, as a production run that read this state
 *      from rv_init.dat would start.  (ljmd_batch_profile_read then describes the warm-up.)
 * Afterwards the handle has a state and valid accelerations; the range flags are cleared, a poison is cleared as
 * ljmd_batch_set_state clears it, the MSD / VACF snapshot numbering restarts at 0 and the accumulators' sums stay.
 * A replica's result depends on its own (n, L, dt, rc, seed, target) only: not on B, its slot or the other replicas.
 * LJMD_ERR_INVALID_ARG, the handle unchanged: NULL seeds or target_total_energy; warmup_steps < 0; a seed of INT32_MIN;
 * a replica whose n is not 4 k^3 ("replica <b>").  LJMD_ERR_INVALID_ARG when target - epot0 <= 0 or ekin0 <= 0 for some
 * replica (the first such "replica <b>" is named): the handle is then left without a state (LJMD_ERR_STATE from the
 * guarded calls until ljmd_batch_set_state or another ljmd_batch_prepare) and is not poisoned.  A failed launch poisons
 * the handle, as elsewhere.
 */
int ljmd_batch_prepare(ljmd_batch_t *h, const int32_t *seeds, const double *target_total_energy,
                       int32_t warmup_steps, double *epot0, double *ekin0);

#ifdef __cplusplus
}
#endif
#endif /* LJMD_H */
