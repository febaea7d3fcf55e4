// ljmd_common.cpp -- error reporting, parameter guards, derived parameters and the device probe shared by the single,
// the multi-device and the batch engine.
#include "ljmd_common.h"

#include <cstdio>

namespace ljmdh {

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

}  // namespace ljmdh
