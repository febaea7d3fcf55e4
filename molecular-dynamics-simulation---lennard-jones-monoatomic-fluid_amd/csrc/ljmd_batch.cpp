// ljmd_batch.cpp -- host side of the batch engine (include/ljmd.h: ljmd_batch_*): B independent replicas of the same
// (n, L, dt, rc) on one device, stepped by one kernel (ljmd_batch.hip) with one workgroup per replica.  Handle
// lifecycle, guards, device state, launch splitting and the combination of the per-replica step records.
#include "ljmd_batch.h"
#include "ljmd_engine.h"

using namespace ljmdb;

struct ljmd_batch {
    int n = 0;
    size_t B = 0;
    int device = 0;
    double L = 0, invL = 0, rc = 0, rc2 = 0, dt = 0, dt_half = 0, dt_sq_half = 0, volume = 0;
    double tail_e = 0, tail_d = 0, tail_dd = 0;
    bool tail_on = true;
    bool have_state = false, have_accel = false;
    bool poisoned = false;            // a launch failed half-way: LJMD_ERR_STATE until ljmd_batch_set_state
    hipStream_t stream = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    double *d_state = nullptr;        // [12][B][n]
    double *d_rec = nullptr;          // [rec_cap][B][kBatchRecWords]
    size_t rec_cap = 0;               // samples the record buffer holds (>= 1)
    std::vector<double> h_rec;
    double last_ms = 0.0;             // kernel time of the last ljmd_batch_steps call
    int32_t last_launches = 0;
    std::string err;
};

namespace {

// pair evaluations per launch: ~15 ms at the estimated 1.3e12 ordered pairs/s of one MI355X (27 fp64 VALU ops per pair,
// DESIGN.md 3.1), so that a launch stays well under 100 ms even at a third of that rate
constexpr double kLaunchPairs = 2e10;
constexpr double kMinParallel = 256;  // below one replica per CU a launch does not get shorter
// ... and a bound for a workgroup that runs alone on its CU, where latency, not throughput, sets the pace: one pass of a
// wave over j costs ~30 dependent fp64 instructions, at most ~100 ns; 2e5 iterations of it per launch = <= 20 ms
constexpr double kLaunchIterations = 2e5;

int bfail(const ljmd_batch *h, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    ljmdh::fail(nullptr, code, "%s", buf);          // the thread's last error, as the single engine
    if (h) const_cast<ljmd_batch *>(h)->err = buf;
    return code;
}

#define BATCH_HIP(h, call)                                                                                  \
    do {                                                                                                    \
        hipError_t e_ = (call);                                                                             \
        if (e_ != hipSuccess)                                                                               \
            return bfail((h), LJMD_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, \
                         __LINE__);                                                                         \
    } while (0)

double *plane(ljmd_batch *h, int which, int axis) { return h->d_state + ((size_t)which * 3 + axis) * h->B * h->n; }

BatchArgs base_args(ljmd_batch *h, int mode)
{
    BatchArgs a{};
    a.state = h->d_state;
    a.rec = h->d_rec;
    a.B = h->B;
    a.n = h->n;
    a.mode = mode;
    a.L = h->L;
    a.invL = h->invL;
    a.rc2 = h->rc2;
    a.dt = h->dt;
    a.dt_half = h->dt_half;
    a.dt_sq_half = h->dt_sq_half;
    return a;
}

// replicas per launch and steps per launch, from the n^2 * steps * max(replicas, CUs) estimate
void launch_shape(const ljmd_batch *h, size_t *chunk, int *steps_per_launch)
{
    const double n2 = (double)h->n * h->n;
    const double c = std::max(kMinParallel, std::floor(kLaunchPairs / n2));
    *chunk = std::min(h->B, (size_t)std::min(c, 2147483647.0));
    const double s = std::floor(kLaunchPairs / (n2 * std::max(kMinParallel, (double)*chunk)));
    const int passes = (batch_k(h->n) + 1) / 2;                 // passes over j per step (ljmd_batch.hip: KG)
    const double s_latency = std::floor(kLaunchIterations / ((double)h->n * passes));
    *steps_per_launch = (int)std::max(1.0, std::min({s, s_latency, (double)LJMD_MAX_PENDING_STEPS}));
}

int ensure_records(ljmd_batch *h, size_t samples)
{
    samples = std::max<size_t>(samples, 1);
    if (samples <= h->rec_cap) return LJMD_OK;
    if (h->d_rec) (void)hipFree(h->d_rec);
    h->d_rec = nullptr;
    h->rec_cap = 0;
    const size_t bytes = samples * h->B * kBatchRecWords * sizeof(double);
    if (hipMalloc(&h->d_rec, bytes) != hipSuccess) {
        h->d_rec = nullptr;
        return bfail(h, LJMD_ERR_ALLOC, "ljmd_batch: cannot allocate %zu bytes of step records", bytes);
    }
    h->rec_cap = samples;
    return LJMD_OK;
}

// copies `samples` records to the host; the handle is poisoned when the kernels behind them failed
int fetch_records(ljmd_batch *h, size_t samples)
{
    h->h_rec.resize(samples * h->B * kBatchRecWords);
    const hipError_t e = hipMemcpyAsync(h->h_rec.data(), h->d_rec, h->h_rec.size() * sizeof(double),
                                        hipMemcpyDeviceToHost, h->stream);
    const hipError_t s = e == hipSuccess ? hipStreamSynchronize(h->stream) : e;
    if (s != hipSuccess) {
        h->poisoned = true;
        return bfail(h, LJMD_ERR_HIP, "ljmd_batch: kernel or copy failed: %s; the handle is poisoned until "
                                      "ljmd_batch_set_state", hipGetErrorString(s));
    }
    return LJMD_OK;
}

// as combine_one (ljmd_capi.cpp) for one replica's record: the kernel already halved the ordered-pair sums
void combine(const ljmd_batch *h, const double *r, double *epot, double *ekin, double *d_epot, double *dd_epot)
{
    const double s12 = r[0], s6 = r[1], kx = r[2], ky = r[3], kz = r[4];
    const double te = h->tail_on ? h->tail_e : 0.0, td = h->tail_on ? h->tail_d : 0.0, tdd = h->tail_on ? h->tail_dd : 0.0;
    if (epot) *epot = 4.0 * (s12 - s6) + te;
    if (d_epot) *d_epot = 24.0 * (-2.0 * s12 + s6) + td;
    if (dd_epot) *dd_epot = 24.0 * (26.0 * s12 - 7.0 * s6) + tdd;
    if (ekin) *ekin = 0.5 * (kx + ky + kz);
}

int upload(ljmd_batch *h, int which, int axis, const double *src)
{
    BATCH_HIP(h, hipMemcpyAsync(plane(h, which, axis), src, h->B * h->n * sizeof(double), hipMemcpyHostToDevice,
                                h->stream));
    return LJMD_OK;
}

}  // namespace

extern "C" {

const char *ljmd_batch_last_error(const ljmd_batch_t *h) { return h ? h->err.c_str() : ljmdh::g_last_error.c_str(); }

int ljmd_batch_create(ljmd_batch_t **out, int32_t n_replicas, int32_t n, double box_length, double dt, double rc,
                      int32_t precision_mode, int32_t device)
{
    if (!out) return bfail(nullptr, LJMD_ERR_INVALID_ARG, "ljmd_batch_create: out is NULL");
    *out = nullptr;
    // the guards of ljmd_create (md_types.f90:143-161), then the batch engine's own
    if (n <= 0) return bfail(nullptr, LJMD_ERR_INVALID_ARG, "ljmd_batch_create: n must be > 0");
    if (!(box_length > 0.0)) return bfail(nullptr, LJMD_ERR_INVALID_ARG, "ljmd_batch_create: box_length must be > 0");
    if (!(rc > 0.0)) return bfail(nullptr, LJMD_ERR_INVALID_ARG, "ljmd_batch_create: rc must be > 0");
    if (rc >= 0.5 * box_length)
        return bfail(nullptr, LJMD_ERR_INVALID_ARG, "ljmd_batch_create: rc must be < L/2 (minimum image convention)");
    if (!(dt > 0.0)) return bfail(nullptr, LJMD_ERR_INVALID_ARG, "ljmd_batch_create: dt must be > 0");
    if (n_replicas < 1) return bfail(nullptr, LJMD_ERR_INVALID_ARG, "ljmd_batch_create: n_replicas must be >= 1");
    if (n > LJMD_BATCH_MAX_N)
        return bfail(nullptr, LJMD_ERR_INVALID_ARG, "ljmd_batch_create: n must be <= LJMD_BATCH_MAX_N (%d)",
                     LJMD_BATCH_MAX_N);
    if (precision_mode != LJMD_PRECISION_FP64)
        return bfail(nullptr, LJMD_ERR_INVALID_ARG, "ljmd_batch_create: precision_mode %d not available for batches "
                                                    "(LJMD_PRECISION_FP64 only)", precision_mode);
    if (!(rc <= (1.0 - 1e-9) * 0.5 * box_length))
        return bfail(nullptr, LJMD_ERR_INVALID_ARG, "ljmd_batch_create: rc must be <= (1 - 1e-9) L/2 (fast-path "
                                                    "precondition; batches have no generic kernel)");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return bfail(nullptr, LJMD_ERR_NO_DEVICE, "ljmd_batch_create: no HIP device available (this library has no CPU path)");
    if (device < 0 || device >= ndev)
        return bfail(nullptr, LJMD_ERR_INVALID_ARG, "ljmd_batch_create: device %d out of range (0..%d)", device, ndev - 1);

    ljmd_batch *h = new (std::nothrow) ljmd_batch;
    if (!h) return bfail(nullptr, LJMD_ERR_ALLOC, "ljmd_batch_create: out of host memory");
    h->n = n;
    h->B = (size_t)n_replicas;
    h->device = device;
    // compute_derived_params, md_types.f90:137-159, the expressions of ljmd_create
    h->L = box_length;
    h->invL = 1.0 / box_length;
    h->volume = box_length * box_length * box_length;
    h->rc = rc;
    h->rc2 = rc * rc;
    h->dt = dt;
    h->dt_half = 0.5 * dt;
    h->dt_sq_half = h->dt_half * dt;
    {   // tail corrections, lj_potential_energy.f90:205-223
        const double npd = (double)n;
        const double rc3 = (rc * rc) * rc;
        const double rc6 = ((rc * rc) * (rc * rc)) * (rc * rc);
        const double tf = 8.0 * ljmdh::kPi * (npd * npd) / (h->volume * rc3);
        h->tail_e = tf * ((1.0 / (3.0 * rc6)) - 1.0) / 3.0;
        h->tail_d = 2.0 * tf * (-2.0 / (3.0 * rc6) + 1.0);
        h->tail_dd = 2.0 * tf * (26.0 / (3.0 * rc6) - 7.0);
    }
    auto undo = [&](int code) {
        const std::string msg = h->err;
        ljmd_batch_destroy(h);
        ljmdh::g_last_error = msg;
        return code;
    };
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreate(&h->ev[0]) != hipSuccess || hipEventCreate(&h->ev[1]) != hipSuccess) {
        bfail(h, LJMD_ERR_HIP, "ljmd_batch_create: cannot create the stream on device %d", device);
        return undo(LJMD_ERR_HIP);
    }
    const size_t bytes = 12 * h->B * (size_t)n * sizeof(double);
    if (hipMalloc(&h->d_state, bytes) != hipSuccess) {
        h->d_state = nullptr;
        bfail(h, LJMD_ERR_ALLOC, "ljmd_batch_create: cannot allocate %zu bytes of replica state", bytes);
        return undo(LJMD_ERR_ALLOC);
    }
    if (ensure_records(h, 1) != LJMD_OK) return undo(LJMD_ERR_ALLOC);
    *out = h;
    return LJMD_OK;
}

void ljmd_batch_destroy(ljmd_batch_t *h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (h->d_state) (void)hipFree(h->d_state);
    if (h->d_rec) (void)hipFree(h->d_rec);
    for (hipEvent_t e : h->ev)
        if (e) (void)hipEventDestroy(e);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

int ljmd_batch_set_state(ljmd_batch_t *h, const double *rx, const double *ry, const double *rz, const double *vx,
                         const double *vy, const double *vz)
{
    if (!h) return bfail(nullptr, LJMD_ERR_INVALID_ARG, "ljmd_batch_set_state: NULL handle");
    if (!rx || !ry || !rz || !vx || !vy || !vz) return bfail(h, LJMD_ERR_INVALID_ARG, "ljmd_batch_set_state: NULL array");
    // fast-path precondition (a), ljmd_kernels.hip: per replica and axis, finite coordinates spanning < 2.4 L
    const double *src[3] = {rx, ry, rz};
    for (size_t b = 0; b < h->B; ++b)
        for (int ax = 0; ax < 3; ++ax) {
            const double *p = src[ax] + b * h->n;
            double lo = INFINITY, hi = -INFINITY;
            for (int i = 0; i < h->n; ++i) {
                lo = std::min(lo, p[i]);
                hi = std::max(hi, p[i]);
                if (!std::isfinite(p[i]))
                    return bfail(h, LJMD_ERR_INVALID_ARG, "ljmd_batch_set_state: replica %zu has a non-finite position", b);
            }
            if (!(hi - lo < 2.4 * h->L))
                return bfail(h, LJMD_ERR_INVALID_ARG, "ljmd_batch_set_state: replica %zu spans >= 2.4 L along axis %d "
                                                      "(wrap the positions first)", b, ax);
        }
    BATCH_HIP(h, hipSetDevice(h->device));
    if (h->poisoned) {
        (void)hipStreamSynchronize(h->stream);   // drain what a failed call left behind
        (void)hipGetLastError();
        h->poisoned = false;
    }
    const double *vs[3] = {vx, vy, vz};
    for (int ax = 0; ax < 3; ++ax) {
        int rc_ = upload(h, LJMD_R, ax, src[ax]);
        if (rc_ == LJMD_OK) rc_ = upload(h, LJMD_RU, ax, src[ax]);    // ru <- r (md_simulation_program.f90:229-231)
        if (rc_ == LJMD_OK) rc_ = upload(h, LJMD_V, ax, vs[ax]);
        if (rc_ != LJMD_OK) return rc_;
    }
    BATCH_HIP(h, hipMemsetAsync(plane(h, LJMD_A, 0), 0, 3 * h->B * h->n * sizeof(double), h->stream));
    BATCH_HIP(h, hipStreamSynchronize(h->stream));
    h->have_state = true;
    h->have_accel = false;
    return LJMD_OK;
}

int ljmd_batch_set_accel(ljmd_batch_t *h, const double *ax, const double *ay, const double *az)
{
    if (!h) return bfail(nullptr, LJMD_ERR_INVALID_ARG, "ljmd_batch_set_accel: NULL handle");
    if (!h->have_state) return bfail(h, LJMD_ERR_STATE, "ljmd_batch_set_accel: call ljmd_batch_set_state first");
    // NULL keeps a component, which is only valid accelerations once there are some: right after set_state every
    // component must be given
    if (!h->have_accel && !(ax && ay && az))
        return bfail(h, LJMD_ERR_INVALID_ARG, "ljmd_batch_set_accel: no valid accelerations to keep; pass all three "
                                              "components (or call ljmd_batch_compute_forces)");
    BATCH_HIP(h, hipSetDevice(h->device));
    const double *src[3] = {ax, ay, az};
    for (int k = 0; k < 3; ++k)
        if (src[k]) {
            const int rc_ = upload(h, LJMD_A, k, src[k]);
            if (rc_ != LJMD_OK) return rc_;
        }
    BATCH_HIP(h, hipStreamSynchronize(h->stream));
    h->have_accel = true;
    return LJMD_OK;
}

int ljmd_batch_set_unwrapped(ljmd_batch_t *h, const double *ux, const double *uy, const double *uz)
{
    if (!h) return bfail(nullptr, LJMD_ERR_INVALID_ARG, "ljmd_batch_set_unwrapped: NULL handle");
    if (!ux || !uy || !uz) return bfail(h, LJMD_ERR_INVALID_ARG, "ljmd_batch_set_unwrapped: NULL array");
    if (!h->have_state) return bfail(h, LJMD_ERR_STATE, "ljmd_batch_set_unwrapped: call ljmd_batch_set_state first");
    BATCH_HIP(h, hipSetDevice(h->device));
    const double *src[3] = {ux, uy, uz};
    for (int k = 0; k < 3; ++k) {
        const int rc_ = upload(h, LJMD_RU, k, src[k]);
        if (rc_ != LJMD_OK) return rc_;
    }
    BATCH_HIP(h, hipStreamSynchronize(h->stream));
    return LJMD_OK;
}

int ljmd_batch_get_state(ljmd_batch_t *h, double *rx, double *ry, double *rz, double *ux, double *uy, double *uz,
                         double *vx, double *vy, double *vz, double *ax, double *ay, double *az)
{
    if (!h) return bfail(nullptr, LJMD_ERR_INVALID_ARG, "ljmd_batch_get_state: NULL handle");
    if (!h->have_state) return bfail(h, LJMD_ERR_STATE, "ljmd_batch_get_state: no state has been set");
    BATCH_HIP(h, hipSetDevice(h->device));
    double *const dst[12] = {rx, ry, rz, ux, uy, uz, vx, vy, vz, ax, ay, az};
    for (int k = 0; k < 12; ++k)
        if (dst[k])
            BATCH_HIP(h, hipMemcpyAsync(dst[k], plane(h, k / 3, k % 3), h->B * h->n * sizeof(double),
                                        hipMemcpyDeviceToHost, h->stream));
    BATCH_HIP(h, hipStreamSynchronize(h->stream));
    return LJMD_OK;
}

int ljmd_batch_compute_forces(ljmd_batch_t *h, double *epot, double *d_epot, double *dd_epot)
{
    if (!h) return bfail(nullptr, LJMD_ERR_INVALID_ARG, "ljmd_batch_compute_forces: NULL handle");
    if (!h->have_state) return bfail(h, LJMD_ERR_STATE, "ljmd_batch_compute_forces: no state has been set");
    if (h->poisoned)
        return bfail(h, LJMD_ERR_STATE, "ljmd_batch_compute_forces: handle poisoned by an earlier failure; call "
                                        "ljmd_batch_set_state");
    BATCH_HIP(h, hipSetDevice(h->device));
    size_t chunk;
    int spl;
    launch_shape(h, &chunk, &spl);
    BatchArgs a = base_args(h, kModeForces);
    for (size_t b0 = 0; b0 < h->B; b0 += chunk) {
        a.b0 = (int)b0;
        const hipError_t e = launch_batch(a, (int)std::min(chunk, h->B - b0), h->stream);
        if (e != hipSuccess) {
            h->poisoned = true;
            return bfail(h, LJMD_ERR_HIP, "ljmd_batch_compute_forces: launch failed: %s", hipGetErrorString(e));
        }
    }
    const int rc_ = fetch_records(h, 1);
    if (rc_ != LJMD_OK) return rc_;
    h->have_accel = true;
    for (size_t b = 0; b < h->B; ++b)
        combine(h, h->h_rec.data() + b * kBatchRecWords, epot ? epot + b : nullptr, nullptr,
                d_epot ? d_epot + b : nullptr, dd_epot ? dd_epot + b : nullptr);
    return LJMD_OK;
}

int ljmd_batch_kinetic_energy(ljmd_batch_t *h, double *ekin)
{
    if (!h || !ekin) return bfail(h, LJMD_ERR_INVALID_ARG, "ljmd_batch_kinetic_energy: NULL argument");
    if (!h->have_state) return bfail(h, LJMD_ERR_STATE, "ljmd_batch_kinetic_energy: no state has been set");
    if (h->poisoned)
        return bfail(h, LJMD_ERR_STATE, "ljmd_batch_kinetic_energy: handle poisoned by an earlier failure; call "
                                        "ljmd_batch_set_state");
    BATCH_HIP(h, hipSetDevice(h->device));
    size_t chunk;
    int spl;
    launch_shape(h, &chunk, &spl);
    BatchArgs a = base_args(h, kModeKinetic);
    for (size_t b0 = 0; b0 < h->B; b0 += chunk) {
        a.b0 = (int)b0;
        const hipError_t e = launch_batch(a, (int)std::min(chunk, h->B - b0), h->stream);
        if (e != hipSuccess) {
            h->poisoned = true;
            return bfail(h, LJMD_ERR_HIP, "ljmd_batch_kinetic_energy: launch failed: %s", hipGetErrorString(e));
        }
    }
    const int rc_ = fetch_records(h, 1);
    if (rc_ != LJMD_OK) return rc_;
    for (size_t b = 0; b < h->B; ++b) ekin[b] = 0.5 * h->h_rec[b * kBatchRecWords + 2];   // md_simulation_program.f90:238-240
    return LJMD_OK;
}

int ljmd_batch_steps(ljmd_batch_t *h, int32_t nsteps, int32_t sample_every, double *epot, double *ekin,
                     double *d_epot, double *dd_epot)
{
    if (!h) return bfail(nullptr, LJMD_ERR_INVALID_ARG, "ljmd_batch_steps: NULL handle");
    if (nsteps < 0) return bfail(h, LJMD_ERR_INVALID_ARG, "ljmd_batch_steps: nsteps < 0");
    const bool sampling = epot || ekin || d_epot || dd_epot;
    if (sampling) {
        if (sample_every < 1) return bfail(h, LJMD_ERR_INVALID_ARG, "ljmd_batch_steps: sample_every must be >= 1");
        if (nsteps % sample_every != 0)
            return bfail(h, LJMD_ERR_INVALID_ARG, "ljmd_batch_steps: nsteps %d is not a multiple of sample_every %d",
                         nsteps, sample_every);
        if (nsteps / sample_every > LJMD_MAX_PENDING_STEPS)
            return bfail(h, LJMD_ERR_INVALID_ARG, "ljmd_batch_steps: %d samples exceed LJMD_MAX_PENDING_STEPS",
                         nsteps / sample_every);
    }
    if (!h->have_state) return bfail(h, LJMD_ERR_STATE, "ljmd_batch_steps: no state has been set");
    if (!h->have_accel)
        return bfail(h, LJMD_ERR_STATE, "ljmd_batch_steps: no valid accelerations; call ljmd_batch_compute_forces or "
                                        "ljmd_batch_set_accel first");
    if (h->poisoned)
        return bfail(h, LJMD_ERR_STATE, "ljmd_batch_steps: handle poisoned by an earlier failure; call "
                                        "ljmd_batch_set_state");
    if (nsteps == 0) return LJMD_OK;
    BATCH_HIP(h, hipSetDevice(h->device));
    const size_t samples = sampling ? (size_t)(nsteps / sample_every) : 0;
    int rc_ = ensure_records(h, samples);
    if (rc_ != LJMD_OK) return rc_;
    size_t chunk;
    int spl;
    launch_shape(h, &chunk, &spl);
    BatchArgs a = base_args(h, kModeSteps);
    a.sample_every = sampling ? sample_every : 0;
    int32_t launches = 0;
    BATCH_HIP(h, hipEventRecord(h->ev[0], h->stream));
    for (int s0 = 0; s0 < nsteps; s0 += spl) {
        a.step0 = s0;
        a.nsteps = std::min(spl, nsteps - s0);
        for (size_t b0 = 0; b0 < h->B; b0 += chunk) {
            a.b0 = (int)b0;
            const hipError_t e = launch_batch(a, (int)std::min(chunk, h->B - b0), h->stream);
            ++launches;
            if (e != hipSuccess) {
                h->poisoned = true;
                return bfail(h, LJMD_ERR_HIP, "ljmd_batch_steps: launch at step %d failed: %s; the handle is poisoned "
                                              "until ljmd_batch_set_state", s0, hipGetErrorString(e));
            }
        }
    }
    BATCH_HIP(h, hipEventRecord(h->ev[1], h->stream));
    rc_ = fetch_records(h, samples);
    if (rc_ != LJMD_OK) return rc_;
    float ms = 0.0f;
    BATCH_HIP(h, hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
    h->last_ms = ms;
    h->last_launches = launches;
    for (size_t s = 0; s < samples; ++s)
        for (size_t b = 0; b < h->B; ++b) {
            const size_t o = s * h->B + b;
            combine(h, h->h_rec.data() + o * kBatchRecWords, epot ? epot + o : nullptr, ekin ? ekin + o : nullptr,
                    d_epot ? d_epot + o : nullptr, dd_epot ? dd_epot + o : nullptr);
        }
    return LJMD_OK;
}

int ljmd_batch_set_tail_corrections(ljmd_batch_t *h, int32_t on)
{
    if (!h) return bfail(nullptr, LJMD_ERR_INVALID_ARG, "ljmd_batch_set_tail_corrections: NULL handle");
    h->tail_on = on != 0;
    return LJMD_OK;
}

int ljmd_batch_profile_read(const ljmd_batch_t *h, double *kernel_ms, int32_t *launches)
{
    if (!h) return bfail(nullptr, LJMD_ERR_INVALID_ARG, "ljmd_batch_profile_read: NULL handle");
    if (kernel_ms) *kernel_ms = h->last_ms;
    if (launches) *launches = h->last_launches;
    return LJMD_OK;
}

}  // extern "C"
