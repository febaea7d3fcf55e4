// ljmd_sort.h -- the two launches that finish a re-sort of the owned shard (ljmd_sort.hip; resort(), ljmd_engine.cpp):
// the lower k-d levels in one kernel, and one gather of everything that follows the permutation.
#ifndef LJMD_SORT_H
#define LJMD_SORT_H

#include <hip/hip_runtime.h>

namespace ljmdk {

// a k-d key = (segment index << kCoordBits) | coordinate quantised to kCoordBits bits, scale = 2^kCoordBits / L
constexpr int kCoordBits = 24;

// A k-d level moves from the library sort into kd_finish_kernel once its largest segment holds at most this many slots:
// one workgroup then owns one segment of that level and sorts it, and every level below it, in LDS (8 bytes per slot for
// the sort + 4 for the slice of the index array: 48 KB).  64 tiles halve to single tiles in 6 levels.
constexpr int kKdFinishCap = 4096;
constexpr int kKdFinishMaxLevels = 6;
constexpr int kKdFinishBlock = 1024;

struct KdFinishArgs {
    const double *pos = nullptr;          // the owned block [3][P]
    int P = 0;
    double scale = 0.0;                   // 2^kCoordBits / L, as kd_level
    const int *idx_in = nullptr;          // permutation after the levels above
    int *idx_out = nullptr;               // ... after the last level; may be idx_in
    const int *offsets = nullptr;         // LaunchPlan::kd_offsets on the device
    int nlevels = 0;                      // levels done here, 1..kKdFinishMaxLevels; one workgroup per segment of the first
    int nseg[kKdFinishMaxLevels] = {};    // LaunchPlan::kd_level_nseg of each
    int off[kKdFinishMaxLevels] = {};     // LaunchPlan::kd_level_off of each
    int axis[kKdFinishMaxLevels] = {};    // split axis of each
};

// r, ru, v (+ a) and the slot -> particle permutation of slot idx[i] to slot i, all in one launch
struct GatherStateArgs {
    const double *src[4] = {};            // [3][P] each; src[3] (a) may be NULL: not gathered
    double *dst[4] = {};
    const int *perm = nullptr;
    int *perm_out = nullptr;
    const int *idx = nullptr;
    int P = 0;
};

// Weak: a host-only harness that links the engine's host files with recording launchers of its own, and never reaches
// a re-sort, need not define them.  resort() fails where one is missing; libljmd.so always holds both.
__attribute__((weak)) hipError_t launch_kd_finish(const KdFinishArgs &a, hipStream_t s);
__attribute__((weak)) hipError_t launch_gather_state(const GatherStateArgs &a, hipStream_t s);

}  // namespace ljmdk
#endif
