// ljmd_series.h -- what the kernels of the engine's resident series observables share with their host side: the argument
// blocks of the kinetic and the fold kernel of the pressure tensor (ljmd_stress.h) and the heat flux (ljmd_heatflux.h),
// and what those kernels' indexing rests on.  The kernels' shared code is ljmd_sum192.h, the host core ljmd_series.cpp.
#ifndef LJMD_SERIES_H
#define LJMD_SERIES_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ljmdk {

// the sums of the particle terms of `block` slots per workgroup
struct SeriesKineticArgs {
    const double *v;                // [3][P] of the own block
    uint64_t *kpart;                // [blocks][particle components][3]
    unsigned *kflag;                // [blocks]
    int P, blocks;
};

struct SeriesFoldArgs {
    const uint64_t *part;           // [workgroups][pair components][3]
    const unsigned long long *pcount;
    const unsigned *pflag;
    const uint64_t *kpart;
    const unsigned *kflag;
    int workgroups, blocks;
    uint64_t *row;                  // [words of a snapshot] of the series: this launch is its only writer
    unsigned long long *count;      // [2] tile pairs of this accumulate
    int32_t *range;                 // sticky
};

inline bool series_kinetic_ok(const SeriesKineticArgs &a, int block)
{
    return a.v && a.kpart && a.kflag && a.P >= 1 && a.blocks >= 1 && (long long)a.blocks * block >= a.P &&
           (long long)(a.blocks - 1) * block < a.P;
}

inline bool series_fold_ok(const SeriesFoldArgs &a)
{
    return a.part && a.pcount && a.pflag && a.kpart && a.kflag && a.row && a.count && a.range && a.workgroups >= 1 &&
           a.blocks >= 1;
}

}  // namespace ljmdk
#endif
