// ljmd_batch.h -- argument block of the batch kernel (ljmd_batch.hip), shared with its host side ljmd_batch.cpp.
//
// Device layout of a batch of B replicas of n particles: twelve planes of B*n doubles, replica-major inside a plane
// (element (b, i) at b*n + i), in the order rx ry rz | ux uy uz | vx vy vz | ax ay az.  Step records: per sample and
// replica kBatchRecWords doubles {0.5 sum u^6, 0.5 sum u^3 over the replica's ordered pairs, sum vx^2, sum vy^2,
// sum vz^2}, sample-major: record (s, b) at (s*B + b) * kBatchRecWords.
#ifndef LJMD_BATCH_KERNEL_H
#define LJMD_BATCH_KERNEL_H

#include <hip/hip_runtime.h>

#include <cstddef>

namespace ljmdb {

constexpr int kBatchRecWords = 5;
constexpr int kBatchMaxThreads = 1024;                 // 16 waves: one workgroup per replica
constexpr int kBatchMaxWaves = kBatchMaxThreads / 64;

enum BatchMode : int {
    kModeForces = 0,    // t = 0 evaluation: a = 24 f, energy sums into record 0 (no drift, no kick)
    kModeSteps = 1,     // nsteps x { drift + wrap + half-kick + unwrapped update ; pair forces ; half-kick }
    kModeKinetic = 2,   // record 0 word 2 = sum (vx*vx + vy*vy + vz*vz), the fused form of ljmd_kinetic_energy
};

struct BatchArgs {
    double *state;          // [12][B][n]
    double *rec;            // [n_samples][B][kBatchRecWords]
    size_t B;               // replicas of the handle (plane stride = B * n)
    int n;
    int b0;                 // first replica of this launch (blockIdx.x + b0)
    int mode;
    int nsteps;             // steps of this launch (kModeSteps)
    int step0;              // steps of the same ljmd_batch_steps call before this launch
    int sample_every;       // step s (1-based within the call) is sampled when s % sample_every == 0; 0 = none
    double L, invL, rc2, dt, dt_half, dt_sq_half;
};


// own particles per thread: 1 up to n = 1024, then 2, then 4 (<= 1024 threads per workgroup)
inline int batch_k(int n) { return n <= 1024 ? 1 : n <= 2048 ? 2 : 4; }
inline int batch_threads(int n)
{
    const int k = batch_k(n);
    return 64 * ((n + 64 * k - 1) / (64 * k));
}

hipError_t launch_batch(const BatchArgs &a, int n_blocks, hipStream_t s);

}  // namespace ljmdb

#endif  // LJMD_BATCH_KERNEL_H
