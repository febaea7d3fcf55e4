// ljmd_heatflux_arith.h -- the device arithmetic of the heat flux (ljmd_heatflux.hip): what a pair within the cutoff
// adds to the six exact integer sums P[3], C[3], what a particle adds to E[3], and the range rule.  The minimum image is
// the pressure tensor's (ljmd_stress_arith.h), included here; add_six and the 192-bit sums are ljmd_sum192.h.
// The definition is include/ljmd.h (ljmd_heatflux_*); compiled with -ffp-contract=off (csrc/Makefile).
#ifndef LJMD_HEATFLUX_ARITH_H
#define LJMD_HEATFLUX_ARITH_H

#include "ljmd_internal.h"
#include "ljmd_stress_arith.h"

namespace ljmdk {

constexpr int kHeatfluxPairTerms = 6;           // P x, y, z, then C x, y, z
constexpr int kHeatfluxKinTerms = 3;            // E x, y, z
static_assert(kHeatfluxPairTerms == 6, "add_six (ljmd_sum192.h) adds the six pair terms");

// One pair within the cutoff, from one side, with w = v_i + v_j: its terms phi w_a (potential) and g d_a (collisional)
// in t; returns whether fx, fy, fz, u6, wx, wy, wz or g is out of range.  add_six(acc, t, <that>, bad) then adds the
// pair.  Under i <-> j w, r2 and phi keep their bits, every d, f and g change sign exactly: t is the same.
__device__ __forceinline__ bool heatflux_terms(double dx, double dy, double dz, double r2, double wx, double wy, double wz,
                                               double (&t)[kHeatfluxPairTerms])
{
    const double u = 1.0 / r2;
    const double u3 = u * u * u;
    const double u6 = u3 * u3;
    const double mdu = 2.0 * u6 - u3;
    const double fx = mdu * dx * u, fy = mdu * dy * u, fz = mdu * dz * u;
    const double phi = u6 - u3;
    const double g = fx * wx + fy * wy + fz * wz;
    t[0] = phi * wx; t[1] = phi * wy; t[2] = phi * wz;
    t[3] = g * dx; t[4] = g * dy; t[5] = g * dz;
    return fixed_out_of_range(fx) || fixed_out_of_range(fy) || fixed_out_of_range(fz) || fixed_out_of_range(u6) ||
           fixed_out_of_range(wx) || fixed_out_of_range(wy) || fixed_out_of_range(wz) || fixed_out_of_range(g);
}

// One particle: acc[a] += Q(k2 v_a) with k2 = vx*vx + vy*vy + vz*vz -- or three zeros, and the flag, when k2 or one of
// the terms is out of range
__device__ __forceinline__ void heatflux_add_kinetic(__int128 (&acc)[kHeatfluxKinTerms], double vx, double vy, double vz, bool &bad)
{
    const double k2 = vx * vx + vy * vy + vz * vz;
    const double t[kHeatfluxKinTerms] = {k2 * vx, k2 * vy, k2 * vz};
    bool oob = fixed_out_of_range(k2);
#pragma unroll
    for (int c = 0; c < kHeatfluxKinTerms; ++c) oob = oob || fixed_out_of_range(t[c]);
    bad = bad || oob;
#pragma unroll
    for (int c = 0; c < kHeatfluxKinTerms; ++c) fixed_add(acc[c], oob ? 0.0 : t[c]);
}

}  // namespace ljmdk
#endif
