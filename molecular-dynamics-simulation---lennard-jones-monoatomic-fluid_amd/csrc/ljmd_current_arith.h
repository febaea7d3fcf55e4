// ljmd_current_arith.h -- the one copy of the arithmetic of the current modes (include/ljmd.h: ljmd_current_*), on top
// of the (C, S) of ljmd_rhok_arith.h: the six products of a (particle, mode) term, its range rule, and the exact split
// of Q.  Everything is fp64 with separate roundings (-ffp-contract=off, csrc/Makefile; no fma() here), the same on the
// device (ljmd_current.hip) and on the host (tests/current_host).
//   P_a = v_a C ; R_a = v_a S                                   (a = x, y, z: one product each, its own rounding)
//   out of range: C or S not finite, or one of the six products not finite or of magnitude >= 2^40 (kFixedBound)
//   Q(t) = RNE(t 2^64), |t| < 2^40: |Q| < 2^104
// Under n -> -n, C keeps its bits and S changes sign (ljmd_rhok_arith.h), and a product with a negated factor is the
// negated product: P_a keeps its bits, R_a changes sign.  A product by +-1 or 2 is exact and Q(2 t) = 2 Q(t).
#ifndef LJMD_CURRENT_ARITH_H
#define LJMD_CURRENT_ARITH_H

#include <hip/hip_runtime.h>

#include "ljmd_rhok_arith.h"

namespace ljmdk {

constexpr double kCurrentBound = 0x1p40;    // kFixedBound (ljmd_internal.h; ljmd_current.hip asserts the two agree)

// t[2 a] = P_a, t[2 a + 1] = R_a: the order of a mode's six sums
__host__ __device__ inline void current_products(double vx, double vy, double vz, double C, double S, double (&t)[6])
{
    t[0] = vx * C; t[1] = vx * S;
    t[2] = vy * C; t[3] = vy * S;
    t[4] = vz * C; t[5] = vz * S;
}

// the whole (particle, mode) term is out of range: it then enters all six sums as zero and sets the range word.  NaN
// fails every comparison, so a product that is not finite is caught by the bound.
__host__ __device__ inline bool current_out_of_range(double C, double S, const double (&t)[6])
{
    bool in = !rhok_out_of_range(C, S);
    for (int k = 0; k < 6; ++k) in = in && __builtin_fabs(t[k]) < kCurrentBound;
    return !in;
}

// Q(t) of |t| < 2^40 in two parts, Q = hi 2^62 + lo -- the split of fixed_add (ljmd_internal.h): v = rint(t 2^64) is an
// integer-valued double, |v| < 2^104; hi = trunc(v 2^-62) has |hi| < 2^42, lo = v - hi 2^62 has |lo| < 2^62 and is a
// multiple of ulp(v), so both are exact and convert exactly.
__host__ __device__ inline void current_fixed_parts(double t, long long &hi, long long &lo)
{
    const double v = __builtin_rint(t * 0x1p64);
    const double h = __builtin_trunc(v * 0x1p-62);
    hi = (long long)h;
    lo = (long long)(v - h * 0x1p62);
}

// acc += Q(t)
__host__ __device__ inline void current_fixed_add(__int128 &acc, double t)
{
    long long hi, lo;
    current_fixed_parts(t, hi, lo);
    acc += (__int128)hi * ((__int128)1 << 62) + (__int128)lo;
}

}  // namespace ljmdk
#endif
