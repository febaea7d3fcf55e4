// ljmd_stress_arith.h -- the one copy of the device arithmetic of the pressure tensor, shared by the single engine's
// kernels (ljmd_stress.hip) and the batch engine's (ljmd_batch_stress.hip): the minimum image, what a pair within the
// cutoff adds to the six exact integer sums, the range rule, and the sum of a 192-bit integer over a wave.
// The definition is include/ljmd.h (ljmd_stress_*); compiled with -ffp-contract=off (csrc/Makefile).
#ifndef LJMD_STRESS_ARITH_H
#define LJMD_STRESS_ARITH_H

#include "ljmd_internal.h"

namespace ljmdk {

constexpr int kStressTerms = 6;                 // xx, yy, zz, xy, xz, yz

// sum over the wave of one signed 192-bit integer per lane; valid in lane 0
__device__ __forceinline__ void wave_sum192(uint64_t (&q)[3])
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        uint64_t o[3];
#pragma unroll
        for (int w = 0; w < 3; ++w) o[w] = __shfl_down(q[w], off, 64);
        add192(q, o);
    }
}

// acc[c] += Q(t[c]) for the six terms -- or six zeros, and the flag, when `oob` or one of the terms is out of range
__device__ __forceinline__ void add_six(__int128 (&acc)[kStressTerms], const double (&t)[kStressTerms], bool oob, bool &bad)
{
#pragma unroll
    for (int c = 0; c < kStressTerms; ++c) oob = oob || fixed_out_of_range(t[c]);
    bad = bad || oob;
#pragma unroll
    for (int c = 0; c < kStressTerms; ++c) fixed_add(acc[c], oob ? 0.0 : t[c]);
}

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
