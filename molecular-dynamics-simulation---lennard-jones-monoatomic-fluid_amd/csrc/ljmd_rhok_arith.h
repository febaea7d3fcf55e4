// ljmd_rhok_arith.h -- the one copy of the arithmetic of the density modes (include/ljmd.h: ljmd_rhok_*): a coordinate
// reduced to turns, and the term (cos, sin) of one particle and one mode.  Everything is fp64 with separate roundings
// (-ffp-contract=off, csrc/Makefile; no fma() here), the same on the device (ljmd_rhok.hip) and on the host
// (tests/rhok_host).
//   t_a = x_a / L ; t_a = t_a - rint(t_a)                       (IEEE division; the subtraction is exact)
//   phi = (n_x t_x + n_y t_y) + n_z t_z ; f = phi - rint(phi)   (exact, |f| <= 1/2)
//   q = rint(4 f) ; g = f - 0.25 q                              (exact, |g| <= 1/8, q in -2 .. 2)
//   th = g 2 pi ; zz = th th ; s, c: odd / even polynomials of degree 15 / 16 in Horner form
//   (q & 3) = 0: (C, S) = (c, s)   1: (-s, c)   2: (-c, -s)   3: (s, -c)
// rint is round-half-even.  Under n -> -n every phi, f, q, g and th changes sign exactly: C keeps its bits, S changes sign.
#ifndef LJMD_RHOK_ARITH_H
#define LJMD_RHOK_ARITH_H

#include <hip/hip_runtime.h>

namespace ljmdk {

constexpr double kRhokTwoPi = 0x1.921fb54442d18p+2;
// the correctly rounded doubles of (-1)^j / (2j + 1)! and (-1)^j / (2j)!
constexpr double kRhokS3 = -0x1.5555555555555p-3, kRhokS5 = 0x1.1111111111111p-7, kRhokS7 = -0x1.a01a01a01a01ap-13,
                 kRhokS9 = 0x1.71de3a556c734p-19, kRhokS11 = -0x1.ae64567f544e4p-26, kRhokS13 = 0x1.6124613a86d09p-33,
                 kRhokS15 = -0x1.ae7f3e733b81fp-41;
constexpr double kRhokC2 = -0x1p-1, kRhokC4 = 0x1.5555555555555p-5, kRhokC6 = -0x1.6c16c16c16c17p-10,
                 kRhokC8 = 0x1.a01a01a01a01ap-16, kRhokC10 = -0x1.27e4fb7789f5cp-22, kRhokC12 = 0x1.1eed8eff8d898p-29,
                 kRhokC14 = -0x1.93974a8c07c9dp-37, kRhokC16 = 0x1.ae7f3e733b81fp-45;

// a coordinate in turns, |t| <= 1/2 (NaN for a coordinate or an L that is not finite)
__host__ __device__ inline double rhok_turns(double x, double L)
{
    const double t = x / L;
    return t - __builtin_rint(t);
}

// (C, S) of the mode (nx, ny, nz), given as doubles, for a particle at (tx, ty, tz) turns
__host__ __device__ inline void rhok_term(double nx, double ny, double nz, double tx, double ty, double tz, double &C, double &S)
{
    const double phi = (nx * tx + ny * ty) + nz * tz;
    const double f = phi - __builtin_rint(phi);
    const double q = __builtin_rint(4.0 * f);
    const double g = f - 0.25 * q;
    const double th = g * kRhokTwoPi, zz = th * th;
    double ps = kRhokS15;
    ps = ps * zz + kRhokS13;
    ps = ps * zz + kRhokS11;
    ps = ps * zz + kRhokS9;
    ps = ps * zz + kRhokS7;
    ps = ps * zz + kRhokS5;
    ps = ps * zz + kRhokS3;
    const double s = th + th * (zz * ps);
    double pc = kRhokC16;
    pc = pc * zz + kRhokC14;
    pc = pc * zz + kRhokC12;
    pc = pc * zz + kRhokC10;
    pc = pc * zz + kRhokC8;
    pc = pc * zz + kRhokC6;
    pc = pc * zz + kRhokC4;
    pc = pc * zz + kRhokC2;
    const double c = 1.0 + zz * pc;
    const int k = q == q ? (int)q & 3 : 0;          // a NaN q: C and S are NaN whatever k
    const bool swap = (k & 1) != 0;
    const double a = swap ? s : c, b = swap ? c : s;
    C = (k == 1 || k == 2) ? -a : a;
    S = (k >= 2) ? -b : b;
}

// a term is out of range when C or S is not finite: it then enters as two zeros and sets the range word.  A finite
// term has |g| <= 1/8, so |C|, |S| < 2.
__host__ __device__ inline bool rhok_out_of_range(double C, double S)
{
    return !(__builtin_fabs(C) < __builtin_inf() && __builtin_fabs(S) < __builtin_inf());
}

// Q(t) = RNE(t 2^64) of |t| <= 2 in two parts, Q = hi 2^32 + lo: v = rint(t 2^64) is an integer-valued double,
// |v| <= 2^65; hi = trunc(v 2^-32) has |hi| <= 2^33, lo = v - hi 2^32 has |lo| < 2^32 and is a multiple of ulp(v), so
// both are exact and convert exactly.  A sum of fewer than 2^29 such parts fits an int64.
__host__ __device__ inline void rhok_fixed_parts(double t, long long &hi, long long &lo)
{
    const double v = __builtin_rint(t * 0x1p64);
    const double h = __builtin_trunc(v * 0x1p-32);
    hi = (long long)h;
    lo = (long long)(v - h * 0x1p32);
}

}  // namespace ljmdk
#endif
