// ljmd_tcf_arith.h -- the one copy of the device arithmetic of the MSD / VACF accumulation, shared by the batch engine's
// kernel (ljmd_batch_tcf.hip) and the single engine's (ljmd_tcf.hip): a term enters an exact integer sum as
// Q(t) = RNE(t 2^64), split into two int64 limbs that a wave sums by integer shuffles and lane 0 adds, as one 128-bit
// integer, into an LDS entry.
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

}  // namespace ljmdk
#endif
