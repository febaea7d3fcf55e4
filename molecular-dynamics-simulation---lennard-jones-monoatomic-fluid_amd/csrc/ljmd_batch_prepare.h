// ljmd_batch_prepare.h -- argument blocks and launchers of the batch engine's on-device initial configurations
// (ljmd_batch_prepare.hip), shared with their host side ljmd_prepare.cpp (include/ljmd.h: ljmd_batch_prepare).
// Same launch geometry as launch_batch (ljmd_batch.h): one workgroup per replica, the handle's replica table, one launch
// per chunk of a kernel class.
#ifndef LJMD_BATCH_PREPARE_H
#define LJMD_BATCH_PREPARE_H

#include "ljmd_batch.h"

namespace ljmdb {

// The generator of the velocities (fortran/random_numbers.f90: the reference's subtractive lagged generator) as
// integers: modulus 4 10^6, seed offset 1618033, lags 55 / 24; a draw is double(m) * (1 / 4e6), the rounded reciprocal.
constexpr int kRanModulus = 4000000;
constexpr int kRanSeedOffset = 1618033;
constexpr int kRanTable = 55;
constexpr int kRanLanes = 24;       // x_j = x_{j-55} - x_{j-24}: 24 consecutive draws depend on earlier rounds only

// FCC lattice in the reference's particle order, 3 n draws of the generator seeded with -|seeds[b]| as velocities - 0.5,
// centre-of-mass velocity R(sum Q(v)) / n removed per axis; writes the planes r, ru (= r) and v of every replica of the
// launch.  A replica's n must be 4 k^3 (the host checks it; the kernel writes no element beyond n either way).
struct BatchInitArgs {
    double *state;              // [12][plane]
    const BatchReplica *rep;
    const int32_t *seeds;       // [B], replica order
    size_t plane;
    int g0;
};
hipError_t launch_batch_init(const BatchInitArgs &a, int n_max, int n_blocks, hipStream_t s);

// v <- v * scale[b], one rounding per component
struct BatchScaleArgs {
    double *state;
    const BatchReplica *rep;
    const double *scale;        // [B], replica order
    size_t plane;
    int g0;
};
hipError_t launch_batch_scale(const BatchScaleArgs &a, int n_max, int n_blocks, hipStream_t s);

}  // namespace ljmdb

#endif  // LJMD_BATCH_PREPARE_H
