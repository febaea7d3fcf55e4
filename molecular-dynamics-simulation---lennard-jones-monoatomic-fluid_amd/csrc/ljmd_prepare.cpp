// ljmd_prepare.cpp -- host side of the batch engine's on-device initial configurations (include/ljmd.h:
// ljmd_batch_prepare; kernels: ljmd_batch_prepare.hip).  The lattice, the velocities and their scaling are this file's
// launches; the energies and the warm-up go through the public ljmd_batch_compute_forces, ljmd_batch_kinetic_energy and
// ljmd_batch_steps, so their launch sequences are the ones a caller of those entry points gets.
// The file name does not match ljmd_batch*.cpp on purpose: the host transcript of the batch engine
// (tests/batch_trace/Makefile) links every such file with launchers of its own, and has none for these kernels.
#include "ljmd_batch_host.h"
#include "ljmd_batch_prepare.h"

#include <climits>

using namespace ljmdb;

namespace {

// k with 4 k^3 == n, or 0
int fcc_cells(int n)
{
    for (int k = 1; 4 * k * k * k <= n; ++k)
        if (4 * k * k * k == n) return k;
    return 0;
}

// the call's two device arrays, released however the call ends
struct PrepareBuffers {
    int32_t *seeds = nullptr;         // [B]
    double *scale = nullptr;          // [B]
    ~PrepareBuffers()
    {
        if (seeds) (void)hipFree(seeds);
        if (scale) (void)hipFree(scale);
    }
};

// one launch per kernel class on the handle's stream; a failure poisons the handle
template <class Launch>
int launch_groups(ljmd_batch *h, const char *who, const char *what, Launch &&launch)
{
    for (const BatchGroup &g : h->groups) {
        const hipError_t e = launch(g);
        if (e != hipSuccess)
            return poison(h, LJMD_ERR_HIP, "%s: %s launch failed: %s; the handle is poisoned until ljmd_batch_set_state", who,
                          what, hipGetErrorString(e));
    }
    return LJMD_OK;
}

int wait(ljmd_batch *h, const char *who)
{
    const hipError_t e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess)
        return poison(h, LJMD_ERR_HIP, "%s: kernel or copy failed: %s; the handle is poisoned until ljmd_batch_set_state", who,
                      hipGetErrorString(e));
    return LJMD_OK;
}

}  // namespace

extern "C" int ljmd_batch_prepare(ljmd_batch_t *h, const int32_t *seeds, const double *target_total_energy,
                                  int32_t warmup_steps, double *epot0, double *ekin0)
{
    static const char *who = "ljmd_batch_prepare";
    LJMD_TRY(enter(h, who, 0));
    if (!seeds || !target_total_energy)
        return fail(h, LJMD_ERR_INVALID_ARG, "%s: seeds and target_total_energy must not be NULL", who);
    if (warmup_steps < 0) return fail(h, LJMD_ERR_INVALID_ARG, "%s: warmup_steps < 0", who);
    for (size_t b = 0; b < h->B; ++b) {
        if (seeds[b] == INT32_MIN)
            return fail(h, LJMD_ERR_INVALID_ARG, "%s: replica %zu: the seed INT32_MIN has no absolute value", who, b);
        if (fcc_cells(h->rep[b].n) == 0)
            return fail(h, LJMD_ERR_INVALID_ARG, "%s: replica %zu: n = %d is not 4 k^3 (no FCC lattice of k^3 cells)", who,
                         b, h->rep[b].n);
    }
    std::vector<double> epot, ekin, scale;
    LJMD_TRY(host_alloc(h, who, [&] {
        epot.resize(h->B);
        ekin.resize(h->B);
        scale.resize(h->B);
    }));
    LJMD_HIP(h, hipSetDevice(h->device));
    PrepareBuffers d;
    LJMD_TRY(device_alloc(h, &d.seeds, h->B * sizeof(int32_t), who, "seeds"));
    LJMD_TRY(device_alloc(h, &d.scale, h->B * sizeof(double), who, "scale factors"));
    if (h->poisoned) {                       // as ljmd_batch_set_state: drain what a failed call left behind
        (void)hipStreamSynchronize(h->stream);
        for (const BatchGroup &g : h->groups)
            if (g.stream) (void)hipStreamSynchronize(g.stream);
        (void)hipGetLastError();
        h->poisoned = false;
    }

    // a, b, c: lattice, velocities, centre of mass; ru <- r.  Accelerations and range flags as ljmd_batch_set_state
    // leaves them
    LJMD_HIP(h, hipMemcpyAsync(d.seeds, seeds, h->B * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    LJMD_HIP(h, hipMemsetAsync(plane(h, LJMD_A, 0), 0, 3 * h->total * sizeof(double), h->stream));
    LJMD_HIP(h, hipMemsetAsync(h->d_range, 0, h->B * sizeof(int32_t), h->stream));
    LJMD_TRY(launch_groups(h, who, "lattice and velocity", [&](const BatchGroup &g) {
        return launch_batch_init(BatchInitArgs{h->d_state, h->d_table, d.seeds, h->total, (int)g.first}, g.n_max,
                                 (int)g.count, h->stream);
    }));
    LJMD_TRY(wait(h, who));
    h->have_state = true;
    h->have_accel = false;
    h->tcf.s = 0;                            // a new trajectory, as after ljmd_batch_set_state
    h->vanhove.s = 0;

    // d: the energies of this state in the handle's mode, the scale factors in IEEE doubles on the host
    LJMD_TRY(ljmd_batch_compute_forces(h, epot.data(), nullptr, nullptr));
    LJMD_TRY(ljmd_batch_kinetic_energy(h, ekin.data()));
    for (size_t b = 0; b < h->B; ++b) {
        const double ekin_new = target_total_energy[b] - epot[b];
        if (!(ekin_new > 0.0) || !(ekin[b] > 0.0)) {
            h->have_state = false;
            h->have_accel = false;
            if (!(ekin_new > 0.0))
                return fail(h, LJMD_ERR_INVALID_ARG, "%s: replica %zu: target_total_energy %.17g leaves no kinetic energy "
                                                      "above epot0 = %.17g; the handle has no state", who, b,
                             target_total_energy[b], epot[b]);
            return fail(h, LJMD_ERR_INVALID_ARG, "%s: replica %zu: ekin0 = %.17g, nothing to rescale; the handle has no "
                                                  "state", who, b, ekin[b]);
        }
        scale[b] = std::sqrt(ekin_new / ekin[b]);
    }
    LJMD_HIP(h, hipMemcpyAsync(d.scale, scale.data(), h->B * sizeof(double), hipMemcpyHostToDevice, h->stream));
    LJMD_TRY(launch_groups(h, who, "scale", [&](const BatchGroup &g) {
        return launch_batch_scale(BatchScaleArgs{h->d_state, h->d_table, d.scale, h->total, (int)g.first}, g.n_max,
                                  (int)g.count, h->stream);
    }));
    LJMD_TRY(wait(h, who));

    // e: the warm-up on the step path, the accumulators' intervals set aside so that it takes no snapshot; ru <- r
    if (warmup_steps > 0) {
        const int32_t rdf_every = h->rdf.every, tcf_every = h->tcf.every, stress_every = h->stress.every,
                      heatflux_every = h->heatflux.every, rhok_every = h->rhok.every;
        h->rdf.every = 0;
        h->tcf.every = 0;
        h->stress.every = 0;
        h->heatflux.every = 0;
        h->rhok.every = 0;
        const int rc_ = ljmd_batch_steps(h, warmup_steps, 1, nullptr, nullptr, nullptr, nullptr);
        h->rdf.every = rdf_every;
        h->tcf.every = tcf_every;
        h->stress.every = stress_every;
        h->heatflux.every = heatflux_every;
        h->rhok.every = rhok_every;
        LJMD_TRY(rc_);
        LJMD_HIP(h, hipMemcpyAsync(plane(h, LJMD_RU, 0), plane(h, LJMD_R, 0), 3 * h->total * sizeof(double),
                                    hipMemcpyDeviceToDevice, h->stream));
        LJMD_TRY(wait(h, who));
    }
    if (epot0) std::copy(epot.begin(), epot.end(), epot0);
    if (ekin0) std::copy(ekin.begin(), ekin.end(), ekin0);
    return LJMD_OK;
}
