// ljmd_stateless.cpp -- the stateless drop-ins of the C ABI: the reference's compute_lj_potential_energy and verlet_step
// signatures on a process-wide cached engine, and the host side of the RDF and time-origin analysis kernels.
#include "ljmd_engine.h"

extern "C" {

namespace {
std::mutex g_cache_mutex;
ljmd_t *g_cached = nullptr;
bool g_stateless_tail_on = true;         // ljmd_stateless_set_tail_corrections: applied to the cached engine of the drop-ins
// what the last ljmd_verlet_step call handed back (r, v, a; 9 n doubles): if the next call passes exactly these
// bytes again -- the reference's own loop only READS the arrays between steps (md_simulation_program.f90:303-353)
// -- the resident state IS the caller's state and the upload + spatial re-sort can be skipped
std::vector<double> g_last_out;
bool g_last_valid = false;

int cached_engine(int32_t n, double L, double dt, double rc, ljmd_t **out)
{
    if (g_cached && (g_cached->n != n || g_cached->L != L || g_cached->rc != rc)) {
        release(g_cached);
        g_cached = nullptr;
        g_last_valid = false;
    }
    if (!g_cached) {
        const int mode = env_int("LJMD_REPRODUCIBLE", 0) != 0 ? LJMD_PRECISION_FP64_REPRODUCIBLE : LJMD_PRECISION_FP64;
        int rc_ = ljmd_create(&g_cached, n, L, dt, rc, mode, env_int("LJMD_DEVICE", 0), 0, 1);
        if (rc_ != LJMD_OK) return rc_;
        g_last_valid = false;
    }
    if (g_cached->dt != dt) {
        if (!(dt > 0.0)) return fail(nullptr, LJMD_ERR_INVALID_ARG, "dt must be > 0");
        g_cached->dt = dt;
        g_cached->dt_half = 0.5 * dt;
        g_cached->dt_sq_half = g_cached->dt_half * dt;
    }
    g_cached->tail_on = g_stateless_tail_on;
    *out = g_cached;
    return LJMD_OK;
}

bool same_as_last_output(size_t n, const double *const a[9])
{
    if (!g_last_valid || g_last_out.size() != 9 * n) return false;
    for (int k = 0; k < 9; ++k)
        if (std::memcmp(a[k], g_last_out.data() + (size_t)k * n, n * sizeof(double)) != 0) return false;
    return true;
}
}  // namespace

int ljmd_compute_lj_potential_energy(int32_t n, double box_length, double rc, const double *rx,
                                     const double *ry, const double *rz, double *ax, double *ay,
                                     double *az, double *epot, double *d_epot, double *dd_epot)
{
    std::lock_guard<std::mutex> lock(g_cache_mutex);
    if (!rx || !ry || !rz || !ax || !ay || !az)  // lj_potential_energy.f90:82
        return fail(nullptr, LJMD_ERR_INVALID_ARG, "compute_lj_potential_energy(): state arrays are not allocated.");
    ljmd_t *h = nullptr;
    int rc_ = cached_engine(n, box_length, 1.0, rc, &h);
    if (rc_ != LJMD_OK) return rc_;
    g_last_valid = false;                        // the resident velocities are about to be overwritten with dummies
    // velocities are irrelevant here; reuse the position arrays as dummies
    if ((rc_ = ljmd_set_state(h, rx, ry, rz, rx, ry, rz)) != LJMD_OK) return rc_;
    if ((rc_ = ljmd_compute_forces(h, epot, d_epot, dd_epot)) != LJMD_OK) return rc_;
    rc_ = ljmd_get_state(h, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                         nullptr, ax, ay, az);
    if (rc_ != LJMD_OK) g_last_error = h->err;
    return rc_;
}

int ljmd_verlet_step(int32_t n, double box_length, double dt, double rc, double *rx, double *ry,
                     double *rz, double *vx, double *vy, double *vz, double *ax, double *ay, double *az,
                     double *epot, double *ekin, double *d_epot, double *dd_epot)
{
    std::lock_guard<std::mutex> lock(g_cache_mutex);
    if (!rx || !ry || !rz || !vx || !vy || !vz || !ax || !ay || !az)  // verlet.f90:52
        return fail(nullptr, LJMD_ERR_INVALID_ARG, "verlet_step(): state arrays are not allocated.");
    ljmd_t *h = nullptr;
    int rc_ = cached_engine(n, box_length, dt, rc, &h);
    if (rc_ != LJMD_OK) return rc_;
    double *const arr[9] = {rx, ry, rz, vx, vy, vz, ax, ay, az};
    const bool resident = env_int("LJMD_STATELESS_FASTPATH", 1) != 0 && !h->poisoned && h->have_state && h->have_accel &&
                          same_as_last_output((size_t)n, arr);
    g_last_valid = false;
    if (!resident) {
        if ((rc_ = ljmd_set_state(h, rx, ry, rz, vx, vy, vz)) != LJMD_OK) return rc_;
        if ((rc_ = ljmd_set_accel(h, ax, ay, az)) != LJMD_OK) return rc_;
    }
    // one step, then the scalar record and the nine arrays behind a single synchronisation
    LJMD_HIP(h, hipSetDevice(h->device));
    rc_ = enqueue_drift(h, nullptr);
    if (rc_ == LJMD_OK) rc_ = enqueue_forces(h, true, nullptr);
    if (rc_ != LJMD_OK) {
        h->poisoned = true;
        g_last_error = h->err;
        return rc_;
    }
    double *const dsts[12] = {rx, ry, rz, nullptr, nullptr, nullptr, vx, vy, vz, ax, ay, az};
    rc_ = download_state(h, dsts, 1);
    if (rc_ != LJMD_OK) {
        g_last_error = h->err;
        return rc_;
    }
    if ((rc_ = combine_records(h, h, h->h_ring, 1, epot, ekin, d_epot, dd_epot)) != LJMD_OK) {
        g_last_error = h->err;
        return rc_;
    }
    g_last_out.resize(9 * (size_t)n);
    for (int k = 0; k < 9; ++k) std::memcpy(g_last_out.data() + (size_t)k * n, arr[k], (size_t)n * sizeof(double));
    g_last_valid = true;
    return LJMD_OK;
}

// ---- trajectory analysis: RDF pair pass -------------------------------------------------

int ljmd_rdf_histogram(int32_t n, const double *x, const double *y, const double *z, double box_length,
                       int32_t nbins, double rmax, uint64_t *hist)
{
    if (n < 2 || !x || !y || !z || !hist || nbins < 1 || nbins > 8192 || !(box_length > 0.0) || !(rmax > 0.0))
        return fail(nullptr, LJMD_ERR_INVALID_ARG, "ljmd_rdf_histogram: bad argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(nullptr, LJMD_ERR_NO_DEVICE, "ljmd_rdf_histogram: no HIP device available (this library has no CPU path)");
    LJMD_HIP(nullptr, hipSetDevice(0));
    double *d = nullptr;
    unsigned long long *dh = nullptr;
    const size_t nb = (size_t)n * sizeof(double);
    auto body = [&]() -> int {
        LJMD_HIP(nullptr, hipMalloc(&d, 3 * nb));
        LJMD_HIP(nullptr, hipMalloc(&dh, (size_t)nbins * sizeof(unsigned long long)));
        LJMD_HIP(nullptr, hipMemcpy(d, x, nb, hipMemcpyHostToDevice));
        LJMD_HIP(nullptr, hipMemcpy(d + n, y, nb, hipMemcpyHostToDevice));
        LJMD_HIP(nullptr, hipMemcpy(d + 2 * (size_t)n, z, nb, hipMemcpyHostToDevice));
        LJMD_HIP(nullptr, hipMemset(dh, 0, (size_t)nbins * sizeof(unsigned long long)));
        RdfArgs a;
        a.x = d;
        a.y = d + n;
        a.z = d + 2 * (size_t)n;
        a.hist = dh;
        a.n = n;
        a.nbins = nbins;
        a.L = box_length;
        a.rmax = rmax;
        a.dr = rmax / nbins;                         // as the reference: dr = rmax / nbins
        a.invL = 1.0 / box_length;
        a.inv_dr = 1.0 / a.dr;
        const int row_blocks = (n + kBlock - 1) / kBlock;
        int ns = std::max(1, std::min((kTargetWorkgroups + row_blocks - 1) / row_blocks, (n + 63) / 64));
        a.chunk = (n + ns - 1) / ns;
        ns = (n + a.chunk - 1) / a.chunk;
        LJMD_HIP(nullptr, launch_rdf_histogram(a, dim3(row_blocks, ns), nullptr));
        std::vector<unsigned long long> hh(nbins);
        LJMD_HIP(nullptr, hipMemcpy(hh.data(), dh, (size_t)nbins * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        for (int b = 0; b < nbins; ++b) hist[b] += hh[b];
        return LJMD_OK;
    };
    const int rc_ = body();
    (void)hipFree(d);
    (void)hipFree(dh);
    return rc_;
}

int ljmd_time_origin_average(int32_t kind, int32_t n_snap, int32_t n, const double *x, const double *y, const double *z,
                             int32_t max_lag, int32_t origin_stride, double *out)
{
    if ((kind != 0 && kind != 1) || n_snap < 2 || n < 1 || !x || !y || !z || !out || max_lag < 0 || origin_stride < 1)
        return fail(nullptr, LJMD_ERR_INVALID_ARG, "ljmd_time_origin_average: bad argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(nullptr, LJMD_ERR_NO_DEVICE, "ljmd_time_origin_average: no HIP device available (this library has no CPU path)");
    LJMD_HIP(nullptr, hipSetDevice(env_int("LJMD_DEVICE", 0)));
    max_lag = std::min(max_lag, n_snap - 1);
    const int n_origins = (n_snap - 1 + origin_stride - 1) / origin_stride;       // t0 = 0, stride, ... < n_snap - 1
    const size_t bytes = (size_t)n_snap * n * sizeof(double), nterm = (size_t)n_origins * (max_lag + 1);
    double *d = nullptr, *dt = nullptr;
    auto body = [&]() -> int {
        LJMD_HIP(nullptr, hipMalloc(&d, 3 * bytes));
        LJMD_HIP(nullptr, hipMalloc(&dt, nterm * sizeof(double)));
        LJMD_HIP(nullptr, hipMemcpy(d, x, bytes, hipMemcpyHostToDevice));
        LJMD_HIP(nullptr, hipMemcpy(d + (size_t)n_snap * n, y, bytes, hipMemcpyHostToDevice));
        LJMD_HIP(nullptr, hipMemcpy(d + 2 * (size_t)n_snap * n, z, bytes, hipMemcpyHostToDevice));
        TimeOriginArgs a;
        a.x = d;
        a.y = d + (size_t)n_snap * n;
        a.z = d + 2 * (size_t)n_snap * n;
        a.term = dt;
        a.n_snap = n_snap;
        a.n = n;
        a.max_lag = max_lag;
        a.origin_stride = origin_stride;
        LJMD_HIP(nullptr, launch_time_origin(a, kind == 1, n_origins, nullptr));
        std::vector<double> term(nterm);
        LJMD_HIP(nullptr, hipMemcpy(term.data(), dt, nterm * sizeof(double), hipMemcpyDeviceToHost));
        // the reference's accumulation: for t0 ascending, acc[:L + 1] += term(t0, :), counts[:L + 1] += 1, then acc / counts
        std::vector<double> acc(max_lag + 1, 0.0);
        std::vector<long> counts(max_lag + 1, 0);
        for (int k = 0; k < n_origins; ++k) {
            const int t0 = k * origin_stride, L = std::min(max_lag, (n_snap - 1) - t0);
            if (L <= 0) continue;
            for (int lag = 0; lag <= L; ++lag) {
                acc[lag] += term[(size_t)k * (max_lag + 1) + lag];
                counts[lag] += 1;
            }
        }
        for (int lag = 0; lag <= max_lag; ++lag) out[lag] = counts[lag] > 0 ? acc[lag] / (double)counts[lag] : 0.0;
        return LJMD_OK;
    };
    const int rc_ = body();
    (void)hipFree(d);
    (void)hipFree(dt);
    return rc_;
}

void ljmd_stateless_set_tail_corrections(int32_t on)
{
    std::lock_guard<std::mutex> lk(g_cache_mutex);
    g_stateless_tail_on = on != 0;
    if (g_cached) g_cached->tail_on = g_stateless_tail_on;
}

void ljmd_stateless_reset(void)
{
    std::lock_guard<std::mutex> lock(g_cache_mutex);
    if (g_cached) release(g_cached);
    g_cached = nullptr;
    g_last_valid = false;
    std::vector<double>().swap(g_last_out);
}

}  // extern "C"
