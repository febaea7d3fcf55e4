// ljmd_tcf_arith.h -- the one copy of the device arithmetic of the MSD / VACF accumulation, shared by the batch engine's
// kernel (ljmd_batch_tcf.hip) and the single engine's (ljmd_tcf.hip): a term enters an exact integer sum as
// Q(t) = RNE(t 2^64), split into two int64 limbs that a wave sums by integer shuffles and lane 0 adds, as one 128-bit
// integer, into an LDS entry; and the two terms of one origin for the particles of a thread (tcf_origin).  The van Hove
// kernels (ljmd_vanhove.hip, ljmd_batch_vanhove.hip) use the limbs and the entries.  What surrounds the arithmetic -- the
// frame of a workgroup, the ring walk, the rows it writes -- is ljmd_origins_dev.h for the single engine's kernels and
// ljmd_batch_origins_dev.h for the batch engine's.
#ifndef LJMD_TCF_ARITH_H
#define LJMD_TCF_ARITH_H

#include "ljmd_internal.h"

namespace ljmdk {

// hi 2^52 + lo += Q(t); an out-of-range term enters as 0
__device__ __forceinline__ void tcf_add(long long &hi, long long &lo, double t, bool &bad)
{
    const bool oob = fixed_out_of_range(t);
    bad = bad || oob;
    const double v = __builtin_rint((oob ? 0.0 : t) * 0x1p64);    // integer-valued, |v| < 2^104
    const double h = __builtin_trunc(v * 0x1p-52);                 // |h| < 2^52
    hi += (long long)h;
    lo += (long long)(v - h * 0x1p52);                             // |.| < 2^52, a multiple of ulp(v): exact
}

__device__ __forceinline__ long long wave_sum_i64(long long v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;  // valid in lane 0
}

// lane 0 of a wave: entry += hi 2^52 + lo as a 128-bit integer {low word, high word}
__device__ __forceinline__ void entry_add(unsigned long long *entry, long long hi, long long lo)
{
    const __int128 x = (__int128)hi * ((__int128)1 << 52) + (__int128)lo;
    const unsigned long long x0 = (unsigned long long)x, x1 = (unsigned long long)(x >> 64);
    const unsigned long long old = atomicAdd(&entry[0], x0);
    const unsigned long long carry = (unsigned long long)(old + x0 < old);
    atomicAdd(&entry[1], x1 + carry);
}

// One origin against the current snapshot, for the K particles of a thread: the MSD and the VACF term of each, summed
// over the wave and added by lane 0 into entry[2 kinds][2 words]; `with0` (uniform across the workgroup): the origin is
// at lag 1, and its lag-0 terms -- the origin against itself -- go to entry0 the same way.  org_of(k, c) loads
// component c of the origin of particle k.
template <int K, class Org>
__device__ __forceinline__ void tcf_origin(const double (&cur)[K][6], Org &&org_of, bool with0, int lane,
                                           unsigned long long *entry, unsigned long long *entry0, bool &bad)
{
    long long m_hi = 0, m_lo = 0, c_hi = 0, c_lo = 0;       // MSD and VACF limbs of this origin
    long long z_hi = 0, z_lo = 0, w_hi = 0, w_lo = 0;       // ... and of its lag 0
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double org[6];
#pragma unroll
        for (int c = 0; c < 6; ++c) org[c] = org_of(k, c);
        const double dx = cur[k][0] - org[0], dy = cur[k][1] - org[1], dz = cur[k][2] - org[2];
        tcf_add(m_hi, m_lo, (dx * dx + dy * dy) + dz * dz, bad);
        tcf_add(c_hi, c_lo, (cur[k][3] * org[3] + cur[k][4] * org[4]) + cur[k][5] * org[5], bad);
        if (with0) {
            const double ex = org[0] - org[0], ey = org[1] - org[1], ez = org[2] - org[2];
            tcf_add(z_hi, z_lo, (ex * ex + ey * ey) + ez * ez, bad);
            tcf_add(w_hi, w_lo, (org[3] * org[3] + org[4] * org[4]) + org[5] * org[5], bad);
        }
    }
    m_hi = wave_sum_i64(m_hi);
    m_lo = wave_sum_i64(m_lo);
    c_hi = wave_sum_i64(c_hi);
    c_lo = wave_sum_i64(c_lo);
    if (with0) {
        z_hi = wave_sum_i64(z_hi);
        z_lo = wave_sum_i64(z_lo);
        w_hi = wave_sum_i64(w_hi);
        w_lo = wave_sum_i64(w_lo);
    }
    if (lane == 0) {
        entry_add(entry, m_hi, m_lo);
        entry_add(entry + 2, c_hi, c_lo);
        if (with0) {
            entry_add(entry0, z_hi, z_lo);
            entry_add(entry0 + 2, w_hi, w_lo);
        }
    }
}

}  // namespace ljmdk
#endif
