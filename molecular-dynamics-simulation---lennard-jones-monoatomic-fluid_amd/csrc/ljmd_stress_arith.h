// ljmd_stress_arith.h -- the one copy of the device arithmetic of the pressure tensor, shared by the single engine's
// kernels (ljmd_stress.hip) and the batch engine's (ljmd_batch_stress.hip): the minimum image, the six terms of a pair
// within the cutoff and their range rule.  How the terms enter the exact integer sums is ljmd_sum192.h.
// The definition is include/ljmd.h (ljmd_stress_*); compiled with -ffp-contract=off (csrc/Makefile).
#ifndef LJMD_STRESS_ARITH_H
#define LJMD_STRESS_ARITH_H

#include "ljmd_internal.h"

namespace ljmdk {

constexpr int kStressTerms = 6;                 // xx, yy, zz, xy, xz, yz

// d = d0 - L * round(d0 * invL), half away from zero
__device__ __forceinline__ double stress_image(double d0, double L, double invL) { return d0 - L * __builtin_round(d0 * invL); }

// One pair within the cutoff, from one side: its six terms f_a d_b in t; returns whether fx, fy, fz or u6 is out of
// range.  add_six(acc, t, <that>, bad) then adds the pair.
__device__ __forceinline__ bool stress_terms(double dx, double dy, double dz, double r2, double (&t)[kStressTerms])
{
    const double u = 1.0 / r2;
    const double u3 = u * u * u;
    const double u6 = u3 * u3;
    const double mdu = 2.0 * u6 - u3;
    const double fx = mdu * dx * u, fy = mdu * dy * u, fz = mdu * dz * u;
    t[0] = fx * dx; t[1] = fy * dy; t[2] = fz * dz;
    t[3] = fx * dy; t[4] = fx * dz; t[5] = fy * dz;
    return fixed_out_of_range(fx) || fixed_out_of_range(fy) || fixed_out_of_range(fz) || fixed_out_of_range(u6);
}

}  // namespace ljmdk
#endif
