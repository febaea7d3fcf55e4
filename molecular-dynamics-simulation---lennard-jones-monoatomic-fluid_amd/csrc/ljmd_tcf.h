// ljmd_tcf.h -- MSD / VACF of the system resident on a one-rank engine (include/ljmd.h: ljmd_tcf_*): argument blocks of
// the three kernels of ljmd_tcf.hip, the sizes of their buffers, and the host core of ljmd_tcf.cpp.
//
// Everything the feature stores is in PARTICLE-ID order (id = index in the arrays of the last ljmd_set_state), padded
// to n_pad = n rounded up to kTcfBlock: cur[6][n_pad] = ru xyz, v xyz of the current snapshot, ring[slots][6][n_pad] the
// stored origins.  Padding elements are zeroed at configure and never written: a padding "particle" yields the terms 0
// and 0, Q(0) = 0, so the terms kernel has no bounds test.  Only the gather kernel sees the slot permutation.
#ifndef LJMD_TCF_H
#define LJMD_TCF_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

namespace ljmdt {

constexpr int kTcfMaxLag = 4096;            // LJMD_TCF_MAX_LAG
constexpr int kTcfMaxOrigins = 512;         // LJMD_TCF_MAX_ORIGINS: ring slots = max_lag / stride + 1
constexpr int kTcfThreads = 256;            // threads of a workgroup of every kernel here
constexpr int kTcfK = 4;                    // particles a thread of the terms kernel owns: tid + k kTcfThreads
constexpr int kTcfBlock = kTcfThreads * kTcfK;   // particle ids per workgroup of the terms kernel
constexpr int kTcfTargetWorkgroups = 1024;  // the live origins are cut into slices until the grid has about this many
constexpr int kTcfMaxChunk = 128;           // live origins per slice at most: its LDS entries, one more for lag 0 ...
constexpr int kTcfLdsBudget = 8 * 1024;     // ... stay inside this many bytes (32 per entry)
static_assert((kTcfMaxChunk + 1) * 32 <= kTcfLdsBudget, "LDS budget of a slice's entries");
constexpr size_t kTcfMaxN = (size_t)1 << 23;   // largest system the sizes below are checked for (tests/tcf_host)

// The window of a snapshot (ljmd_tcf_host.h: TcfWindow): origin e = 0 .. n_live - 1 at lag lag_first - e stride in ring
// slot (slot_first + e) % slots; entry n_live is the lag-0 entry of the newest origin, present when that origin is at
// lag 1.  Slice y of the grid takes the origins [y chunk, min(n_live, (y + 1) chunk)); the last slice the lag-0 entry.

struct TcfGatherArgs {
    const double *ru, *v;   // [3][P] slot order
    const int *perm;        // [P] slot -> particle id (>= n on padding slots)
    double *cur;            // [6][n_pad] particle-id order
    double *store;          // the ring slot [6][n_pad] that takes this snapshot, or NULL
    int n, P;
    size_t n_pad;
};

struct TcfTermsArgs {
    const double *cur;              // [6][n_pad]
    const double *ring;             // [slots][6][n_pad]
    unsigned long long *part;       // [nblk][ents][2 kinds][2 words]: rows of block x, entries of slice y
    int32_t *flag;                  // [nblk][slots]: element (x, y) = 1 when a term of that workgroup was out of range
    size_t n_pad;
    int nblk, slots, ents, stride;  // ents = slots + 1: up to `slots` live origins and the lag-0 entry
    int n_live, lag_first, slot_first;
    int chunk, slices;
};

struct TcfFoldArgs {
    const unsigned long long *part;
    const int32_t *flag;
    uint64_t *sums;                 // [2][max_lag + 1][3] signed 192-bit: kind 0 = MSD, 1 = VACF
    int32_t *range;                 // sticky word
    int nblk, slots, ents, stride, max_lag;
    int n_live, lag_first;
    int chunk, slices;
};

hipError_t launch_tcf_gather(const TcfGatherArgs &a, hipStream_t s);
hipError_t launch_tcf_terms(const TcfTermsArgs &a, hipStream_t s);
hipError_t launch_tcf_fold(const TcfFoldArgs &a, hipStream_t s);

// ---- host core (ljmd_tcf.cpp): knows nothing of struct ljmd ----

// what the core needs to know of an engine
struct TcfView {
    int n = 0, P = 0, G = 1;        // G = n_ranks (a multi-device handle: its number of devices)
    bool multi = false;
    const double *ru = nullptr, *v = nullptr;   // [3][P]
    const int *perm = nullptr;      // the DEVICE's permutation, stream-ordered behind the re-sorts
    hipStream_t stream = nullptr;
};

// sizes of one configuration, all in size_t: the ring of n = 262 144 with 512 slots has 6.4e9 bytes
struct TcfSizes {
    int slots = 0, ents = 0, nblk = 0;  // ents = slots + 1 entries per row of the partials
    size_t n_pad = 0;
    size_t cur_bytes = 0, ring_bytes = 0, part_bytes = 0, flag_bytes = 0, sums_bytes = 0;
};
TcfSizes tcf_sizes(int n, int max_lag, int stride);

// the grid of the terms kernel for n_live >= 1 live origins: (nblk, slices), chunk origins per slice
struct TcfSlices {
    int chunk = 0, slices = 0;
};
TcfSlices tcf_plan_slices(int nblk, int n_live);

struct TcfState {
    int max_lag = 0;                // 0 = not configured
    int stride = 0, n = 0;
    TcfSizes sz;
    double *d_cur = nullptr, *d_ring = nullptr;
    unsigned long long *d_part = nullptr;
    int32_t *d_flag = nullptr, *d_range = nullptr;
    uint64_t *d_sums = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;    // around the launches of the most recent accumulate
    bool timed = false;
    int last_live = 0;              // live origins the most recent accumulate visited
    int64_t s = 0;                  // number of the next snapshot of this trajectory
    int64_t snapshots = 0;
    std::vector<int64_t> counts;    // [max_lag + 1] origins that contributed to each lag
};

// All return an LJMD_* code and leave a message in *err (and in the thread's last error).  `who` = the public name.
int tcf_configure(TcfState *st, std::string *err, const char *who, const TcfView &v, int32_t max_lag, int32_t origin_stride);
int tcf_accumulate(TcfState *st, std::string *err, const char *who, const TcfView &v);
// waits for the device; LJMD_ERR_RANGE while the sticky word is set; words [2][max_lag + 1][3] or NULL
int tcf_fetch(TcfState *st, std::string *err, const char *who, const TcfView &v, uint64_t *words, int64_t *counts,
              int64_t *n_snapshots);
int tcf_read(TcfState *st, std::string *err, const char *who, const TcfView &v, double *msd, double *vacf, int64_t *counts,
             int64_t *n_snapshots);
int tcf_reset(TcfState *st, std::string *err, const char *who, const TcfView &v);
int tcf_profile_read(TcfState *st, std::string *err, const char *who, const TcfView &v, double *kernel_ms,
                     int32_t *origins_live);
// ljmd_set_state: the stored origins are dropped and the numbering restarts; sums and counts stay
void tcf_new_trajectory(TcfState *st);
// frees everything after what may still use it; the state is "not configured" afterwards
void tcf_release(TcfState *st, hipStream_t stream);

}  // namespace ljmdt
#endif
