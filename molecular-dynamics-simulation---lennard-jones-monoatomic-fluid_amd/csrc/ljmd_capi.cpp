// ljmd_capi.cpp -- the C ABI of the stateful single / sharded engine declared in include/ljmd.h: entry checks,
// dispatch to the multi-device driver (ljmd_multi.cpp), and calls into the engine (ljmd_engine.h).
//
// The engine owns the HBM-resident simulation state and sequences the gfx950 kernels of
// ljmd_kernels.hip / ljmd_sort.hip on one HIP stream.  There is no CPU compute path in
// this library: without a HIP device every compute entry point returns
// LJMD_ERR_NO_DEVICE.
#include "ljmd_engine.h"
#include "ljmd_multi.h"

#include <new>

namespace ljmdh {

int entry_checks(const ljmd_t *h, const char *who, unsigned checks)
{
    if ((checks & kHandle) && !h) return fail(nullptr, LJMD_ERR_INVALID_ARG, "%s: NULL handle", who);
    if ((checks & kHaveState) && !h->have_state) return fail(h, LJMD_ERR_STATE, "%s: no state has been set", who);
    if ((checks & kHaveAccel) && !h->have_accel)
        return fail(h, LJMD_ERR_STATE, "%s: accelerations not initialised (call ljmd_compute_forces first)", who);
    if ((checks & kNotPoisoned) && h->poisoned)
        return fail(h, LJMD_ERR_STATE, "%s: handle poisoned by an earlier failure; call ljmd_set_state", who);
    return LJMD_OK;
}

}  // namespace ljmdh

// ---------------------------------------------------------------------------
extern "C" {

const char *ljmd_version(void) { return "ljmd 0.6.0 gfx950"; }

int32_t ljmd_device_count(void)
{
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess) return 0;
    return c;
}

const char *ljmd_last_error(const ljmd_t *h) { return h ? h->err.c_str() : g_last_error.c_str(); }

int ljmd_create(ljmd_t **out, int32_t n, double box_length, double dt, double rc,
                int32_t precision_mode, int32_t device, int32_t rank, int32_t n_ranks)
{
    if (!out) return fail(nullptr, LJMD_ERR_INVALID_ARG, "ljmd_create: out is NULL");
    *out = nullptr;
    LJMD_TRY(check_sim_params("ljmd_create", n, box_length, dt, rc));
    if (precision_mode != LJMD_PRECISION_FP64 && precision_mode != LJMD_PRECISION_FP32_FORCE &&
        precision_mode != LJMD_PRECISION_FP64_REPRODUCIBLE)
        return fail(nullptr, LJMD_ERR_INVALID_ARG, "ljmd_create: precision_mode %d not available", precision_mode);
    if (precision_mode == LJMD_PRECISION_FP64_REPRODUCIBLE && n > kFixedMaxN)
        return fail(nullptr, LJMD_ERR_INVALID_ARG, "ljmd_create: LJMD_PRECISION_FP64_REPRODUCIBLE takes n <= %d", kFixedMaxN);
    if (n_ranks < 1 || rank < 0 || rank >= n_ranks)
        return fail(nullptr, LJMD_ERR_INVALID_ARG, "ljmd_create: bad rank %d of %d", rank, n_ranks);
    if (n % n_ranks != 0)
        return fail(nullptr, LJMD_ERR_INVALID_ARG, "ljmd_create: n=%d not divisible by n_ranks=%d", n, n_ranks);
    LJMD_TRY(probe_device(device, "ljmd_create"));

    ljmd_t *h = new (std::nothrow) ljmd;
    if (!h) return fail(nullptr, LJMD_ERR_ALLOC, "ljmd_create: out of host memory");
    h->n = n;
    h->G = n_ranks;
    h->rank = rank;
    h->device = device;
    h->mode = precision_mode;
    static_cast<SimParams &>(*h) = derive_params(n, box_length, dt, rc);
    h->knobs = read_knobs();
    h->inject_failure_at = h->knobs.inject_failure_at_step;
    int rc_ = plan_engine(*h, n, n_ranks, precision_mode, h->knobs, &h->plan);
    if (rc_ != LJMD_OK) {
        delete h;
        return rc_;
    }
    h->h_perm.resize(h->plan.P);
    for (int i = 0; i < h->plan.P; ++i) h->h_perm[i] = i;
    rc_ = allocate_engine(h);
    if (rc_ != LJMD_OK) {
        g_last_error = h->err;
        release(h);
        return rc_;
    }
    *out = h;
    return LJMD_OK;
}

void ljmd_destroy(ljmd_t *h)
{
    if (h && h->multi)
        ljmdm::destroy(h);
    else
        release(h);
}

int ljmd_create_multi(ljmd_t **out, int32_t n, double box_length, double dt, double rc, int32_t precision_mode,
                      int32_t n_gpus, const int32_t *devices)
{
    return ljmdm::create(out, n, box_length, dt, rc, precision_mode, n_gpus, devices);
}

// ---- state transfer --------------------------------------------------------

int ljmd_set_state(ljmd_t *h, const double *rx, const double *ry, const double *rz,
                   const double *vx, const double *vy, const double *vz)
{
    LJMD_TRY(entry_checks(h, "ljmd_set_state", kHandle));
    if (!rx || !ry || !rz || !vx || !vy || !vz)
        return fail(h, LJMD_ERR_INVALID_ARG, "ljmd_set_state: NULL array");
    if (h->multi) return ljmdm::set_state(h, rx, ry, rz, vx, vy, vz);
    h->boxes_valid = false;
    h->drift_prefused = false;
    h->step_open = false;
    ljmdt::tcf_new_trajectory(&h->tcf);     // resident MSD / VACF: the origins are dropped, sums and counts stay
    ljmdv::vanhove_new_trajectory(&h->vanhove);     // van Hove: likewise
    LJMD_HIP(h, hipSetDevice(h->device));
    if (h->poisoned) {
        // a batch of steps failed half-way: drain the stream, forget whatever records were in flight and take the
        // device's own count of finished steps as the truth
        LJMD_HIP(h, hipStreamSynchronize(h->stream));
        LJMD_HIP(h, hipMemcpy(&h->ring_issued, h->d_ring_pos, sizeof(unsigned), hipMemcpyDeviceToHost));
        h->ring_consumed = h->ring_issued;
        h->forces_pending = false;
        h->gather_done_for_step = false;
        h->fold_pending = false;            // (a record a failed batch left to its next tail launch)
        h->poisoned = false;
    }
    const size_t S = h->plan.S, P = h->plan.P;
    // all n positions into the exchange buffer in original order, NaN on the padding;
    // track the coordinate spread (fast-path precondition (a), ljmd_kernels.hip)
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    const double *src[3] = {rx, ry, rz};
    bool finite = true;
    for (int g = 0; g < h->G; ++g)
        for (int ax = 0; ax < 3; ++ax) {
            double *dst = h->h_stage + ((size_t)g * 3 + ax) * P;
            const double *s = src[ax] + (size_t)g * S;
            for (size_t i = 0; i < S; ++i) {
                const double x = s[i];
                dst[i] = x;
                lo[ax] = std::min(lo[ax], x);
                hi[ax] = std::max(hi[ax], x);
                finite = finite && std::isfinite(x);
            }
            for (size_t i = S; i < P; ++i) dst[i] = NAN;
        }
    // Fast-path precondition (a): the tile-pair test (axis_gap, uniform_image) and the pair kernels take coordinate
    // differences |d| < 2.5 L.  Kernels that read the coordinates as given (gather, fixed-point, g(r) and stress walks)
    // have that for a span < 2.4 L: positions_compact.  The Newton-3 kernels read them framed per row group
    // (tile_boxes_kernel: every particle in the image nearest to the first particle of its group, so up to L / 2 beyond
    // either end of the span where a group is wider than L / 2, as groups of raw input can be), and differences of framed
    // coordinates reach span + L.  From a span of 1.4 L on (positions_wide) the frame is therefore taken from the wrapped
    // coordinates, which keeps the framed copy inside [-L / 2, 3 L / 2] whatever the input.
    h->positions_compact = finite;
    h->positions_wide = false;
    for (int ax = 0; ax < 3; ++ax) {
        if (!(hi[ax] - lo[ax] < 2.4 * h->L)) h->positions_compact = false;
        if (!(hi[ax] - lo[ax] < 1.4 * h->L)) h->positions_wide = true;
    }
    {   // k-d split axes: halve the longest remaining extent of the OWN shard at every level, so that a
        // slab- or column-shaped shard (multi-GPU index ranges) still ends in near-cubic tiles
        double ext[3];
        for (int ax = 0; ax < 3; ++ax) {
            double slo = INFINITY, shi = -INFINITY;
            const double *sp = src[ax] + (size_t)h->rank * S;
            for (size_t i = 0; i < S; ++i) {
                slo = std::min(slo, sp[i]);
                shi = std::max(shi, sp[i]);
            }
            ext[ax] = std::isfinite(shi - slo) ? std::min(shi - slo, h->L) : h->L;
            if (!(ext[ax] > 0.0)) ext[ax] = 1e-300;
        }
        h->kd_axis.assign(h->plan.kd_level_nseg.size(), 0);
        for (size_t l = 0; l < h->kd_axis.size(); ++l) {
            int best = 0;
            for (int ax = 1; ax < 3; ++ax)
                if (ext[ax] > ext[best] * (1.0 + 1e-9)) best = ax;   // ties -> lowest axis: x, y, z cycling for a cube
            h->kd_axis[l] = best;
            ext[best] *= 0.5;
        }
    }
    LJMD_HIP(h, hipMemcpyAsync(h->d_pos, h->h_stage, 3 * P * h->G * sizeof(double), hipMemcpyHostToDevice,
                               h->stream));
    // ru <- r (md_simulation_program.f90:229-231), own shard
    LJMD_HIP(h, hipMemcpyAsync(h->d_ru, own_block(h), 3 * P * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    LJMD_HIP(h, hipMemsetAsync(h->d_a, 0, 3 * P * sizeof(double), h->stream));
    LJMD_HIP(h, hipStreamSynchronize(h->stream));
    // slot order is the original order again, and the shard is the caller's index range again
    h->migrated = false;
    LJMD_HIP(h, launch_iota_offset(h->d_gid0, h->plan.S, h->plan.P, h->rank * h->plan.S, h->stream));
    for (int i = 0; i < h->plan.P; ++i) h->h_perm[i] = i;
    LJMD_HIP(h, hipMemcpyAsync(h->d_perm, h->h_perm.data(), P * sizeof(int), hipMemcpyHostToDevice, h->stream));
    h->perm_dirty = false;
    int rc_ = upload_shard3(h, h->d_v, vx, vy, vz);
    if (rc_ != LJMD_OK) return rc_;
    h->have_state = true;
    h->have_accel = false;
    if (h->plan.sort_enabled && fast_path_ok(h)) {
        rc_ = resort(h, false);   // accelerations are all zero at this point
        if (rc_ != LJMD_OK) return rc_;
    }
    return LJMD_OK;
}

int ljmd_set_accel(ljmd_t *h, const double *ax, const double *ay, const double *az)
{
    LJMD_TRY(entry_checks(h, "ljmd_set_accel", kHandle));
    if (!ax || !ay || !az) return fail(h, LJMD_ERR_INVALID_ARG, "ljmd_set_accel: NULL array");
    if (h->multi) return ljmdm::set_accel(h, ax, ay, az);
    if (!h->have_state) return fail(h, LJMD_ERR_STATE, "ljmd_set_accel: call ljmd_set_state first");
    LJMD_HIP(h, hipSetDevice(h->device));
    const int rc_ = upload_shard3(h, h->d_a, ax, ay, az);
    if (rc_ == LJMD_OK) h->have_accel = true;
    return rc_;
}

int ljmd_set_unwrapped(ljmd_t *h, const double *ux, const double *uy, const double *uz)
{
    LJMD_TRY(entry_checks(h, "ljmd_set_unwrapped", kHandle));
    if (!ux || !uy || !uz) return fail(h, LJMD_ERR_INVALID_ARG, "ljmd_set_unwrapped: NULL array");
    if (h->multi) return ljmdm::set_unwrapped(h, ux, uy, uz);
    if (!h->have_state) return fail(h, LJMD_ERR_STATE, "ljmd_set_unwrapped: call ljmd_set_state first");
    LJMD_HIP(h, hipSetDevice(h->device));
    return upload_shard3(h, h->d_ru, ux, uy, uz);
}

int ljmd_get_state(ljmd_t *h, double *rx, double *ry, double *rz, double *ux, double *uy, double *uz,
                   double *vx, double *vy, double *vz, double *ax, double *ay, double *az)
{
    LJMD_TRY(entry_checks(h, "ljmd_get_state", kHandle | kHaveState));
    if (h->multi) {
        double *const p[12] = {rx, ry, rz, ux, uy, uz, vx, vy, vz, ax, ay, az};
        return ljmdm::get_state(h, p);
    }
    LJMD_HIP(h, hipSetDevice(h->device));
    double *const dsts[12] = {rx, ry, rz, ux, uy, uz, vx, vy, vz, ax, ay, az};
    return download_state(h, dsts, 0);
}

// ---- hot path ----------------------------------------------------------------

int ljmd_compute_forces(ljmd_t *h, double *epot, double *d_epot, double *dd_epot)
{
    LJMD_TRY(entry_checks(h, "ljmd_compute_forces", kHandle | kHaveState | kNotPoisoned));
    if (h->multi) return ljmdm::compute_forces(h, epot, d_epot, dd_epot);
    if (h->G != 1)
        return fail(h, LJMD_ERR_STATE, "ljmd_compute_forces: sharded engine; use ljmd_forces_partial");
    LJMD_HIP(h, hipSetDevice(h->device));
    EventSet *q = next_events(h);
    if (q) LJMD_HIP(h, hipEventRecord(q->e[0], h->stream));
    const bool keep = h->want_energy;
    h->want_energy = true;                      // this call exists to return the three sums
    int rc_ = enqueue_forces(h, false, q);
    h->want_energy = keep;
    if (rc_ != LJMD_OK) return rc_;
    rc_ = fetch_ring(h, 1);
    if (rc_ != LJMD_OK) return rc_;
    return combine_records(h, h, h->h_ring, 1, epot, nullptr, d_epot, dd_epot);
}

namespace {
// what ljmd_verlet_steps and ljmd_enqueue_steps[_sampled] check before anything is enqueued
int steps_entry(const ljmd_t *h, int32_t nsteps, const char *who)
{
    LJMD_TRY(entry_checks(h, who, kHandle));
    if (nsteps < 0) return fail(h, LJMD_ERR_INVALID_ARG, "%s: nsteps < 0", who);
    LJMD_TRY(entry_checks(h, who, kHaveState | kHaveAccel | kNotPoisoned));
    if (!h->multi && h->G != 1) return fail(h, LJMD_ERR_STATE, "%s: sharded engine; use ljmd_step_begin/finish", who);
    return LJMD_OK;
}

// nsteps x (drift + forces) behind one another, nothing read back.  sampled: only the LAST of the nsteps evaluates the
// potential-energy sums (the step the reference samples, md_simulation_program.f90:361); positions, velocities,
// accelerations and ekin do not depend on them.  ring_guard: the records already pending must survive this batch
int enqueue_steps(ljmd_t *h, int32_t nsteps, bool sampled, const char *who, bool ring_guard)
{
    if (h->multi) return ljmdm::enqueue_steps(h, nsteps, sampled);
    static_assert(LJMD_MAX_PENDING_STEPS == kRingCap, "LJMD_MAX_PENDING_STEPS out of sync with the record ring");
    if (ring_guard && (h->ring_issued - h->ring_consumed) + (unsigned)nsteps > kRingCap)
        return fail(h, LJMD_ERR_STATE, "%s: %u + %d pending steps exceed LJMD_MAX_PENDING_STEPS", who,
                    h->ring_issued - h->ring_consumed, nsteps);
    LJMD_HIP(h, hipSetDevice(h->device));
    const bool keep = h->want_energy;
    for (int s = 0; s < nsteps; ++s) {
        EventSet *q = next_events(h);
        if (sampled) h->want_energy = s == nsteps - 1;
        int rc_ = enqueue_drift(h, q);
        if (rc_ == LJMD_OK) rc_ = enqueue_forces(h, true, q, s + 1 < nsteps);
        if (rc_ != LJMD_OK) {
            h->want_energy = keep;
            h->poisoned = true;      // a step is half enqueued: no rollback, the state is no longer a trajectory point
            return rc_;
        }
    }
    h->want_energy = keep;
    return LJMD_OK;
}

// the records of the last nsteps steps, combined into the caller's arrays (NULL = not wanted)
int collect_steps(ljmd_t *h, int32_t nsteps, double *epot, double *ekin, double *d_epot, double *dd_epot, const char *who)
{
    LJMD_TRY(entry_checks(h, who, kHandle));
    if (nsteps < 0 || nsteps > (int)kRingCap) return fail(h, LJMD_ERR_INVALID_ARG, "%s: nsteps out of range", who);
    LJMD_TRY(entry_checks(h, who, kNotPoisoned));
    if (h->multi) return ljmdm::collect_steps(h, nsteps, epot, ekin, d_epot, dd_epot);
    if (h->G != 1) return fail(h, LJMD_ERR_STATE, "%s: sharded engine; use ljmd_read_partials", who);
    LJMD_HIP(h, hipSetDevice(h->device));
    LJMD_TRY(fetch_ring(h, (unsigned)nsteps));
    for (int s = 0; s < nsteps; ++s)
        LJMD_TRY(combine_records(h, h, h->h_ring + (size_t)s * h->rec_stride, 1, epot ? epot + s : nullptr,
                                 ekin ? ekin + s : nullptr, d_epot ? d_epot + s : nullptr, dd_epot ? dd_epot + s : nullptr));
    return LJMD_OK;
}
}  // namespace

int ljmd_verlet_steps(ljmd_t *h, int32_t nsteps, double *epot, double *ekin, double *d_epot,
                      double *dd_epot)
{
    static const char *who = "ljmd_verlet_steps";
    LJMD_TRY(steps_entry(h, nsteps, who));
    // nobody reads the potential-energy sums (the warm-up of the initial-configuration driver): forces-only pair kernel
    const bool keep = h->want_energy, wanted = keep && (epot || d_epot || dd_epot);
    ljmd_set_observables(h, wanted);
    int rc_ = LJMD_OK;
    for (int done = 0; done < nsteps && rc_ == LJMD_OK;) {      // batches the record ring holds; each is collected at once
        const int batch = std::min<int>(nsteps - done, (int)kRingCap);
        rc_ = enqueue_steps(h, batch, false, who, false);
        if (rc_ == LJMD_OK)
            rc_ = collect_steps(h, batch, epot ? epot + done : nullptr, ekin ? ekin + done : nullptr,
                                d_epot ? d_epot + done : nullptr, dd_epot ? dd_epot + done : nullptr, who);
        done += batch;
    }
    ljmd_set_observables(h, keep);
    return rc_;
}

// ---- asynchronous production loop ---------------------------------------------

int ljmd_enqueue_steps(ljmd_t *h, int32_t nsteps)
{
    LJMD_TRY(steps_entry(h, nsteps, "ljmd_enqueue_steps"));
    return enqueue_steps(h, nsteps, false, "ljmd_enqueue_steps", true);
}

int ljmd_enqueue_steps_sampled(ljmd_t *h, int32_t nsteps)
{
    LJMD_TRY(steps_entry(h, nsteps, "ljmd_enqueue_steps"));     // (its messages name ljmd_enqueue_steps)
    return enqueue_steps(h, nsteps, true, "ljmd_enqueue_steps", true);
}

int ljmd_set_observables(ljmd_t *h, int32_t on)
{
    LJMD_TRY(entry_checks(h, "ljmd_set_observables", kHandle));
    if (h->multi) return ljmdm::set_observables(h, on != 0);
    h->want_energy = on != 0;
    return LJMD_OK;
}

int ljmd_collect_steps(ljmd_t *h, int32_t nsteps, double *epot, double *ekin, double *d_epot, double *dd_epot)
{
    return collect_steps(h, nsteps, epot, ekin, d_epot, dd_epot, "ljmd_collect_steps");
}

int ljmd_snapshot_begin(ljmd_t *h)
{
    LJMD_TRY(entry_checks(h, "ljmd_snapshot_begin", kHandle | kHaveState));
    if (h->multi) return ljmdm::snapshot_begin(h);
    if (h->snap_in_flight)
        return fail(h, LJMD_ERR_STATE, "ljmd_snapshot_begin: a snapshot is already in flight (call ljmd_snapshot_end)");
    LJMD_HIP(h, hipSetDevice(h->device));
    const size_t P3 = 3 * (size_t)h->plan.P * sizeof(double), PI = (size_t)h->plan.P * sizeof(int);
    if (!h->snap_ready) {
        // lazily, once; a failure part-way leaves snap_ready false and the next call resumes where this one stopped
        // (release() frees whatever exists)
        if (!h->copy_stream) LJMD_HIP(h, hipStreamCreateWithFlags(&h->copy_stream, hipStreamNonBlocking));
        if (!h->ev_snap_ready) LJMD_HIP(h, hipEventCreateWithFlags(&h->ev_snap_ready, hipEventDisableTiming));
        if (!h->ev_snap_done) LJMD_HIP(h, hipEventCreateWithFlags(&h->ev_snap_done, hipEventDisableTiming));
        if (!h->d_snap) LJMD_HIP(h, hipMalloc(&h->d_snap, 4 * P3));
        if (!h->d_snap_perm) LJMD_HIP(h, hipMalloc(&h->d_snap_perm, PI));
        if (!h->h_snap) LJMD_HIP(h, hipHostMalloc(&h->h_snap, 4 * P3, hipHostMallocDefault));
        if (!h->h_snap_perm) LJMD_HIP(h, hipHostMalloc(&h->h_snap_perm, PI, hipHostMallocDefault));
        h->snap_ready = true;
    }
    // 1. engine stream: freeze the state as of the steps enqueued so far (HBM -> HBM, ~100 N bytes)
    const double *srcs[4] = {own_block(h), h->d_ru, h->d_v, h->d_a};
    for (int w = 0; w < 4; ++w)
        LJMD_HIP(h, hipMemcpyAsync(h->d_snap + (size_t)w * 3 * h->plan.P, srcs[w], P3, hipMemcpyDeviceToDevice, h->stream));
    LJMD_HIP(h, hipMemcpyAsync(h->d_snap_perm, h->d_perm, PI, hipMemcpyDeviceToDevice, h->stream));
    LJMD_HIP(h, hipEventRecord(h->ev_snap_ready, h->stream));
    // 2. copy stream: HBM -> pinned host, concurrent with whatever the engine stream runs next
    LJMD_HIP(h, hipStreamWaitEvent(h->copy_stream, h->ev_snap_ready, 0));
    LJMD_HIP(h, hipMemcpyAsync(h->h_snap, h->d_snap, 4 * P3, hipMemcpyDeviceToHost, h->copy_stream));
    LJMD_HIP(h, hipMemcpyAsync(h->h_snap_perm, h->d_snap_perm, PI, hipMemcpyDeviceToHost, h->copy_stream));
    LJMD_HIP(h, hipEventRecord(h->ev_snap_done, h->copy_stream));
    h->snap_in_flight = true;
    return LJMD_OK;
}

int ljmd_snapshot_end(ljmd_t *h, double *rx, double *ry, double *rz, double *ux, double *uy, double *uz,
                      double *vx, double *vy, double *vz, double *ax, double *ay, double *az)
{
    LJMD_TRY(entry_checks(h, "ljmd_snapshot_end", kHandle));
    if (h->multi) {
        double *const p[12] = {rx, ry, rz, ux, uy, uz, vx, vy, vz, ax, ay, az};
        return ljmdm::snapshot_end(h, p);
    }
    if (!h->snap_in_flight) return fail(h, LJMD_ERR_STATE, "ljmd_snapshot_end: no snapshot in flight");
    LJMD_HIP(h, hipSetDevice(h->device));
    LJMD_HIP(h, hipEventSynchronize(h->ev_snap_done));      // the transfer only, not the engine's stream
    h->snap_in_flight = false;
    const size_t P = h->plan.P;
    double *dsts[4][3] = {{rx, ry, rz}, {ux, uy, uz}, {vx, vy, vz}, {ax, ay, az}};
    for (int w = 0; w < 4; ++w)
        for (int k = 0; k < 3; ++k) {
            double *dst = dsts[w][k];
            if (!dst) continue;
            const double *st = h->h_snap + ((size_t)w * 3 + k) * P;
            for (size_t i = 0; i < P; ++i) {
                const int o = h->h_snap_perm[i];
                if (o < h->plan.S) dst[o] = st[i];              // slot -> original index of the shard
            }
        }
    return LJMD_OK;
}

int ljmd_kinetic_energy(ljmd_t *h, double *ekin)
{
    if (!h || !ekin) return fail(h, LJMD_ERR_INVALID_ARG, "ljmd_kinetic_energy: NULL argument");
    LJMD_TRY(entry_checks(h, "ljmd_kinetic_energy", kHaveState));
    if (h->multi) return ljmdm::kinetic_energy(h, ekin);
    LJMD_HIP(h, hipSetDevice(h->device));
    if (reproducible(h)) {                       // 0.5 ((Kx + Ky) + Kz), exact sums; per-rank part when sharded
        int64_t rec[kExactWords];
        const int rc_ = kinetic_exact(h, rec);
        if (rc_ != LJMD_OK) return rc_;
        return combine_exact(h, rec, 1, nullptr, ekin, nullptr, nullptr);
    }
    LJMD_HIP(h, launch_kinetic_fused(integrate_args(h), h->stream));
    std::vector<double> part(3 * (size_t)h->plan.n_ke);
    LJMD_HIP(h, hipMemcpyAsync(part.data(), h->d_ke_part, part.size() * sizeof(double),
                               hipMemcpyDeviceToHost, h->stream));
    LJMD_HIP(h, hipStreamSynchronize(h->stream));
    double s = 0.0;
    for (int b = 0; b < h->plan.n_ke; ++b) s += part[3 * (size_t)b];
    *ekin = 0.5 * s;  // per-rank partial when sharded
    return LJMD_OK;
}

// ---- multi-GPU split phase ---------------------------------------------------

int ljmd_shard_range(const ljmd_t *h, int32_t *i0, int32_t *i1)
{
    LJMD_TRY(entry_checks(h, "ljmd_shard_range", kHandle));
    if (h->multi) return fail(h, LJMD_ERR_STATE, "ljmd_shard_range: a multi-device handle runs the exchange phases itself");
    // after an ownership migration the rank owns a SET of particles, not an index range: stitching rank arrays together
    // by [i0, i1) would silently permute the state
    if (h->migrated)
        return fail(h, LJMD_ERR_STATE, "ljmd_shard_range: this rank has migrated since ljmd_set_state and owns the "
                                       "particles ljmd_particle_ids names, not an index range");
    if (i0) *i0 = h->rank * h->plan.S;
    if (i1) *i1 = (h->rank + 1) * h->plan.S;
    return LJMD_OK;
}

void *ljmd_exchange_buffer(ljmd_t *h, int64_t *n_total, int64_t *own_off, int64_t *own_cnt)
{
    if (!h || h->multi) return nullptr;
    if (n_total) *n_total = 3 * (int64_t)h->plan.P * h->G;
    if (own_off) *own_off = (int64_t)h->rank * 3 * h->plan.P;
    if (own_cnt) *own_cnt = 3 * (int64_t)h->plan.P;
    return h->d_pos;
}

void *ljmd_device_ptr(ljmd_t *h, int32_t which, int32_t axis)
{
    if (!h || h->multi || axis < 0 || axis > 2) return nullptr;
    double *base = nullptr;
    switch (which) {
        case LJMD_R: base = own_block(h); break;
        case LJMD_RU: base = h->d_ru; break;
        case LJMD_V: base = h->d_v; break;
        case LJMD_A: base = h->d_a; break;
        default: return nullptr;
    }
    return base + (size_t)axis * h->plan.P;
}

void *ljmd_stream(ljmd_t *h) { return (h && !h->multi) ? (void *)h->stream : nullptr; }

int ljmd_step_begin(ljmd_t *h)
{
    LJMD_TRY(entry_checks(h, "ljmd_step_begin", kHandle));
    if (h->multi) return fail(h, LJMD_ERR_STATE, "ljmd_step_begin: a multi-device handle runs the exchange phases itself");
    if (!h->have_state || !h->have_accel)
        return fail(h, LJMD_ERR_STATE, "ljmd_step_begin: state/accelerations not initialised");
    LJMD_HIP(h, hipSetDevice(h->device));
    h->step_open = true;                 // the own block runs ahead of the exchange buffer until ljmd_step_finish
    return enqueue_drift(h, next_events(h));
}

int ljmd_step_forces(ljmd_t *h)
{
    LJMD_TRY(entry_checks(h, "ljmd_step_forces", kHandle));
    if (h->multi) return fail(h, LJMD_ERR_STATE, "ljmd_step_forces: a multi-device handle runs the exchange phases itself");
    LJMD_TRY(entry_checks(h, "ljmd_step_forces", kHaveState));
    LJMD_HIP(h, hipSetDevice(h->device));
    // pairs with the event set taken by ljmd_step_begin (the last one handed out)
    EventSet *q = (h->profiling && h->ev_used > 0) ? &h->ev_pool[h->ev_used - 1] : nullptr;
    return enqueue_pair_forces(h, q);
}

int ljmd_step_finish(ljmd_t *h)
{
    LJMD_TRY(entry_checks(h, "ljmd_step_finish", kHandle));
    if (h->multi) return fail(h, LJMD_ERR_STATE, "ljmd_step_finish: a multi-device handle runs the exchange phases itself");
    LJMD_TRY(entry_checks(h, "ljmd_step_finish", kHaveState));
    LJMD_HIP(h, hipSetDevice(h->device));
    EventSet *q = (h->profiling && h->ev_used > 0) ? &h->ev_pool[h->ev_used - 1] : nullptr;
    if (!h->forces_pending) {
        const int rc_ = enqueue_pair_forces(h, q);
        if (rc_ != LJMD_OK) return rc_;
    }
    const int rc_ = enqueue_kick(h, true, q);
    if (rc_ == LJMD_OK) h->step_open = false;
    return rc_;
}

int ljmd_force_buffers(ljmd_t *h, int32_t external, void **fpart, int64_t *fpart_doubles, void **frecv,
                       int64_t *frecv_doubles)
{
    LJMD_TRY(entry_checks(h, "ljmd_force_buffers", kHandle));
    if (h->multi) return fail(h, LJMD_ERR_STATE, "ljmd_force_buffers: a multi-device handle runs the exchange phases itself");
    h->external_force_exchange = external != 0;
    if (fpart) *fpart = h->d_fpart;
    if (fpart_doubles) *fpart_doubles = 3 * (int64_t)h->plan.P * (needs_force_exchange(h) ? h->G : 1);
    if (frecv) *frecv = h->d_frecv;
    if (frecv_doubles) *frecv_doubles = needs_force_exchange(h) ? 3 * (int64_t)h->plan.P : 0;
    return LJMD_OK;
}

int ljmd_forces_partial(ljmd_t *h)
{
    LJMD_TRY(entry_checks(h, "ljmd_forces_partial", kHandle));
    if (h->multi) return fail(h, LJMD_ERR_STATE, "ljmd_forces_partial: a multi-device handle runs the exchange phases itself");
    LJMD_TRY(entry_checks(h, "ljmd_forces_partial", kHaveState));
    LJMD_HIP(h, hipSetDevice(h->device));
    if (!h->forces_pending) {
        const int rc_ = enqueue_pair_forces(h, nullptr);
        if (rc_ != LJMD_OK) return rc_;
    }
    return enqueue_kick(h, false, nullptr);
}

int ljmd_read_partials(ljmd_t *h, int32_t nsteps, double *partial)
{
    if (!h || !partial || nsteps < 0 || nsteps > (int)kRingCap)
        return fail(h, LJMD_ERR_INVALID_ARG, "ljmd_read_partials: bad argument");
    if (h->multi) return fail(h, LJMD_ERR_STATE, "ljmd_read_partials: a multi-device handle combines its ranks itself");
    if (reproducible(h))
        return fail(h, LJMD_ERR_STATE, "ljmd_read_partials: reproducible handle; use ljmd_read_partials_exact");
    LJMD_HIP(h, hipSetDevice(h->device));
    int rc_ = fetch_ring(h, (unsigned)nsteps);
    if (rc_ != LJMD_OK) return rc_;
    std::memcpy(partial, h->h_ring, (size_t)nsteps * kPartialStride * sizeof(double));
    return LJMD_OK;
}

int ljmd_read_partials_exact(ljmd_t *h, int32_t nsteps, int64_t *words)
{
    if (!h || !words || nsteps < 0 || nsteps > (int)kRingCap)
        return fail(h, LJMD_ERR_INVALID_ARG, "ljmd_read_partials_exact: bad argument");
    if (h->multi) return fail(h, LJMD_ERR_STATE, "ljmd_read_partials_exact: a multi-device handle combines its ranks itself");
    if (!reproducible(h))
        return fail(h, LJMD_ERR_STATE, "ljmd_read_partials_exact: not a LJMD_PRECISION_FP64_REPRODUCIBLE handle");
    LJMD_HIP(h, hipSetDevice(h->device));
    int rc_ = fetch_ring(h, (unsigned)nsteps);
    if (rc_ != LJMD_OK) return rc_;
    std::memcpy(words, h->h_ring, (size_t)nsteps * kExactWords * sizeof(int64_t));
    return LJMD_OK;
}

int ljmd_combine_scalars_exact(const ljmd_t *h, const int64_t *words_by_rank, int32_t n_ranks, double *epot,
                               double *ekin, double *d_epot, double *dd_epot)
{
    if (!h || !words_by_rank || n_ranks < 1)
        return fail(nullptr, LJMD_ERR_INVALID_ARG, "ljmd_combine_scalars_exact: bad argument");
    if (!reproducible(h))
        return fail(h, LJMD_ERR_STATE, "ljmd_combine_scalars_exact: not a LJMD_PRECISION_FP64_REPRODUCIBLE handle");
    return combine_exact(h, words_by_rank, n_ranks, epot, ekin, d_epot, dd_epot);
}

int ljmd_combine_scalars(const ljmd_t *h, const double *partials_by_rank, int32_t n_ranks, double *epot,
                         double *ekin, double *d_epot, double *dd_epot)
{
    if (!h || !partials_by_rank || n_ranks < 1)
        return fail(nullptr, LJMD_ERR_INVALID_ARG, "ljmd_combine_scalars: bad argument");
    if (reproducible(h))
        return fail(h, LJMD_ERR_STATE, "ljmd_combine_scalars: reproducible handle; use ljmd_combine_scalars_exact");
    combine_one(h, partials_by_rank, n_ranks, epot, ekin, d_epot, dd_epot);
    return LJMD_OK;
}

// ---- RCCL exchange (one process per GPU) -------------------------------------

int ljmd_comm_unique_id(char *id_out)
{
    if (!id_out) return fail(nullptr, LJMD_ERR_INVALID_ARG, "ljmd_comm_unique_id: NULL buffer");
    static_assert(sizeof(ncclUniqueId) == LJMD_COMM_ID_BYTES, "LJMD_COMM_ID_BYTES out of sync with RCCL");
    ncclUniqueId id;
    const ncclResult_t r = ncclGetUniqueId(&id);
    if (r != ncclSuccess) return fail(nullptr, LJMD_ERR_HIP, "ncclGetUniqueId failed: %s", ncclGetErrorString(r));
    std::memcpy(id_out, id.internal, sizeof id.internal);
    return LJMD_OK;
}

int ljmd_comm_init(ljmd_t *h, const char *id)
{
    if (!h || !id) return fail(h, LJMD_ERR_INVALID_ARG, "ljmd_comm_init: NULL argument");
    if (h->multi) return fail(h, LJMD_ERR_STATE, "ljmd_comm_init: a multi-device handle owns its communicators");
    if (h->comm) return fail(h, LJMD_ERR_STATE, "ljmd_comm_init: communicator already initialised");
    LJMD_HIP(h, hipSetDevice(h->device));
    ncclUniqueId uid;
    std::memcpy(uid.internal, id, sizeof uid.internal);
    const ncclResult_t r = ncclCommInitRank(&h->comm, h->G, uid, h->rank);
    if (r != ncclSuccess) {
        h->comm = nullptr;
        return fail(h, LJMD_ERR_HIP, "ncclCommInitRank(rank %d of %d) failed: %s", h->rank, h->G, ncclGetErrorString(r));
    }
    LJMD_HIP(h, hipStreamCreateWithFlags(&h->comm_stream, hipStreamNonBlocking));
    LJMD_HIP(h, hipEventCreateWithFlags(&h->ev_pos_ready, hipEventDisableTiming));
    LJMD_HIP(h, hipEventCreateWithFlags(&h->ev_gather_done, hipEventDisableTiming));
    return LJMD_OK;
}

int ljmd_set_tail_corrections(ljmd_t *h, int32_t on)
{
    LJMD_TRY(entry_checks(h, "ljmd_set_tail_corrections", kHandle));
    // host-side only: the constants are added when the step records are combined (combine_one), on the handle the
    // caller holds -- for a multi-device handle that is the parent
    h->tail_on = on != 0;
    return LJMD_OK;
}

int32_t ljmd_multi_migrations(const ljmd_t *h)
{
    return !h ? 0 : h->multi ? ljmdm::migrations(h) : h->migrations;
}

int32_t ljmd_comm_size(const ljmd_t *h)
{
    if (h && h->multi) return ljmdm::comm_size(h);
    if (!h || !h->comm) return 0;
    int count = 0;
    if (ncclCommCount(h->comm, &count) != ncclSuccess) return 0;
    return count;
}

int ljmd_allgather_positions(ljmd_t *h)
{
    LJMD_TRY(entry_checks(h, "ljmd_allgather_positions", kHandle));
    if (h->multi) return fail(h, LJMD_ERR_STATE, "ljmd_allgather_positions: a multi-device handle runs the exchange phases itself");
    if (h->G == 1 && !h->knobs.force_collectives) return LJMD_OK;
    if (!h->comm) return fail(h, LJMD_ERR_STATE, "ljmd_allgather_positions: call ljmd_comm_init first");
    LJMD_HIP(h, hipSetDevice(h->device));
    if (h->gather_done_for_step) {       // already issued by ljmd_step_begin on the communication stream
        h->gather_done_for_step = false;
        return LJMD_OK;
    }
    // serial form (t = 0, re-sort steps, LJMD_OVERLAP_EXCHANGE=0): behind the drift/kick (and re-sort) kernels
    // and ahead of the pair kernel
    EventSet *q = (h->profiling && h->ev_used > 0) ? &h->ev_pool[h->ev_used - 1] : nullptr;
    const bool cs = use_comm_stream(h);
    const hipStream_t xs = cs ? h->comm_stream : h->stream;
    int rc_ = cs ? comm_begin(h) : LJMD_OK;
    if (rc_ != LJMD_OK) return rc_;
    if (q) LJMD_HIP(h, hipEventRecord(q->e[5], xs));
    rc_ = allgather_on(h, xs);
    if (rc_ != LJMD_OK) return rc_;
    if (q) {
        LJMD_HIP(h, hipEventRecord(q->e[6], xs));
        q->has_pos_x = true;
    }
    return cs ? comm_end(h) : LJMD_OK;
}

int ljmd_memcpy(ljmd_t *h, void *dst, const void *src, int64_t bytes, int32_t kind)
{
    if (!h || !dst || !src || bytes < 0 || kind < 1 || kind > 3)
        return fail(h, LJMD_ERR_INVALID_ARG, "ljmd_memcpy: bad argument");
    if (h->multi) return fail(h, LJMD_ERR_STATE, "ljmd_memcpy: not available on a multi-device handle");
    LJMD_HIP(h, hipSetDevice(h->device));
    const hipMemcpyKind k = kind == 1 ? hipMemcpyHostToDevice : kind == 2 ? hipMemcpyDeviceToHost
                                                                           : hipMemcpyDeviceToDevice;
    LJMD_HIP(h, hipMemcpyAsync(dst, src, (size_t)bytes, k, h->stream));
    LJMD_HIP(h, hipStreamSynchronize(h->stream));
    return LJMD_OK;
}

int ljmd_synchronize(ljmd_t *h)
{
    LJMD_TRY(entry_checks(h, "ljmd_synchronize", kHandle));
    if (h->multi) return ljmdm::synchronize(h);
    LJMD_HIP(h, hipSetDevice(h->device));
    LJMD_HIP(h, hipStreamSynchronize(h->stream));
    LJMD_HIP(h, hipDeviceSynchronize());
    return LJMD_OK;
}

}  // extern "C"
