// ljmd_resident.h -- host side of the seven observables of the system resident on the single / sharded engine: g(r)
// (ljmd_rdf.cpp); the pressure tensor (ljmd_stress.cpp) and the heat flux (ljmd_heatflux.cpp), which are two descriptors
// over the one series core (ljmd_series.cpp); MSD / VACF (ljmd_tcf.cpp) and the van Hove self-correlation
// (ljmd_vanhove.cpp), which are two descriptors over the one time-origin core (ljmd_origins.cpp); the density modes
// (ljmd_rhok.cpp); the current modes (ljmd_current.cpp).  What the cores share
// -- the view through which they see an engine, their named device buffers, the timer around one accumulate -- and each
// core's state and functions.  A core knows nothing of struct ljmd and links without the engine (tests/rdf_host,
// tests/tcf_host, tests/stress_host, tests/heatflux_host, tests/vanhove_host, tests/rhok_host, tests/current_host); every
// C entry point that takes a handle is in ljmd_resident.cpp.  Host code only: the kernels' side is ljmd_rdf.h,
// ljmd_stress.h, ljmd_heatflux.h, ljmd_rhok.h, ljmd_current.h, ljmd_tcf.h and ljmd_vanhove.h, the latter two over
// ljmd_origins.h.
#ifndef LJMD_RESIDENT_H
#define LJMD_RESIDENT_H

#include "ljmd_common.h"
#include "ljmd_current.h"
#include "ljmd_heatflux.h"
#include "ljmd_rdf.h"
#include "ljmd_rhok.h"
#include "ljmd_stress.h"
#include "ljmd_tcf.h"
#include "ljmd_tcf_host.h"
#include "ljmd_vanhove.h"

#include <array>
#include <optional>
#include <string>
#include <vector>

namespace ljmdh {

// what the cores need to know of an engine; each reads the fields of its own kernels
struct ResidentView {
    int n = 0, S = 0, P = 0, TB = 0, T = 0, G = 1, rank = 0;   // G = n_ranks (a multi-device handle: its number of devices)
    bool multi = false;
    double L = 0, invL = 0, rc2 = 0;
    const double *pos = nullptr;    // exchange buffer
    const double *ru = nullptr, *v = nullptr;   // [3][P]
    const int *perm = nullptr;      // the DEVICE's permutation, stream-ordered behind the re-sorts
    hipStream_t stream = nullptr;
    bool compact = false;           // coordinate spread < 2.4 L
    std::optional<int> walk_chunk;  // LJMD_WALK_CHUNK as the handle read it (Knobs::walk_chunk)
    std::optional<int> vanhove_chunk;   // LJMD_VANHOVE_CHUNK as the handle read it (Knobs::vanhove_chunk)
};

// one device buffer of a state: where its pointer lives, its size, and what a failed allocation calls it
struct DeviceBuffer {
    void **p;
    size_t bytes;
    const char *name;
};

// allocates in the order of the list; the buffer that fails stays NULL: "<who>: out of device memory for <name>"
template <class Buffers>
int alloc_buffers(std::string *err, const char *who, const Buffers &bufs)
{
    for (const DeviceBuffer &b : bufs)
        if (hipMalloc(b.p, b.bytes) != hipSuccess) {
            *b.p = nullptr;
            (void)hipGetLastError();
            return fail(err, LJMD_ERR_ALLOC, "%s: out of device memory for %s (%zu bytes)", who, b.name, b.bytes);
        }
    return LJMD_OK;
}

// frees what exists, after what may still use it on `stream`
template <class Buffers>
void free_buffers(const Buffers &bufs, hipStream_t stream)
{
    bool any = false;
    for (const DeviceBuffer &b : bufs) any = any || *b.p;
    if (stream && any) (void)hipStreamSynchronize(stream);
    for (const DeviceBuffer &b : bufs)
        if (*b.p) (void)hipFree(*b.p);
}

// device time of the launches of the most recent accumulate
struct KernelTimer {
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timed = false;             // ev0 / ev1 have been recorded

    hipError_t create()
    {
        const hipError_t e = hipEventCreate(&ev0);
        return e != hipSuccess ? e : hipEventCreate(&ev1);
    }
    void destroy()
    {
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        *this = {};
    }
    hipError_t start(hipStream_t s) { return hipEventRecord(ev0, s); }
    hipError_t stop(hipStream_t s)
    {
        const hipError_t e = hipEventRecord(ev1, s);
        if (e == hipSuccess) timed = true;
        return e;
    }
    // waits for `s`; 0 before the first accumulate
    hipError_t elapsed_ms(hipStream_t s, float *ms) const
    {
        *ms = 0.0f;
        if (!timed) return hipSuccess;
        const hipError_t e = hipStreamSynchronize(s);
        return e != hipSuccess ? e : hipEventElapsedTime(ms, ev0, ev1);
    }
};

}  // namespace ljmdh

// Every core function returns an LJMD_* code and leaves a message in *err (and in the thread's last error).  `who` = the
// public name.  *_release frees everything after what may still use it; the state is "not configured" afterwards.
// not_configured fails with LJMD_ERR_STATE and the observable's "... is not configured" message.

namespace ljmdr {

using ljmdh::ResidentView;

struct RdfState {
    int nbins = 0;                  // 0 = not configured
    double rmax = 0, dr = 0, inv_dr = 0;
    unsigned long long *d_hist = nullptr;   // [nbins]
    unsigned long long *d_count = nullptr;  // [2]
    double *d_bbox = nullptr;               // [T][kRdfBoxStride]
    ljmdh::KernelTimer timer;
    int64_t snapshots = 0;
};

// the grid of one accumulate: steps, steps per slice, slices
struct RdfWalk {
    int U = 0, chunk = 0, slices = 0, row_blocks = 0, weight = 0;
};
// walk_chunk unset: steps per slice by kRdfTargetWorkgroups; set: that many, clamped to [1, min(U, kRdfMaxChunk)] (tests)
RdfWalk rdf_plan_walk(int TB, int T, int G, std::optional<int> walk_chunk = std::nullopt);

int not_configured(std::string *err, const char *who);
int rdf_configure(RdfState *st, std::string *err, const char *who, const ResidentView &v, int32_t nbins, double rmax);
int rdf_accumulate(RdfState *st, std::string *err, const char *who, const ResidentView &v);
int rdf_read(RdfState *st, std::string *err, const char *who, const ResidentView &v, uint64_t *hist, int64_t *n_snapshots);
int rdf_reset(RdfState *st, std::string *err, const char *who, const ResidentView &v);
int rdf_profile_read(RdfState *st, std::string *err, const char *who, const ResidentView &v, int64_t *visited, int64_t *total,
                     double *kernel_ms);
void rdf_release(RdfState *st, hipStream_t stream);

}  // namespace ljmdr

// The time-origin observables -- MSD / VACF and the van Hove self-correlation: one state, one core (ljmd_origins.cpp), and
// a constant descriptor of each observable (ljmd_tcf.cpp, ljmd_vanhove.cpp) that the core is driven by.  Snapshot
// numbering, window, counts and quotient are ljmd_tcf_host.h's.  The histogram fields are 0 / NULL without a histogram.
namespace ljmdh {

// sizes of one configuration, all in size_t: the ring of n = 262 144 with 512 slots and 6 components has 6.4e9 bytes
struct OriginSizes {
    int slots = 0, ents = 0, nblk = 0;  // ents = slots + 1 entries per row of the partials
    size_t n_pad = 0;
    size_t cur_bytes = 0, ring_bytes = 0, part_bytes = 0, flag_bytes = 0, sums_bytes = 0, hist_bytes = 0;
};

// the grid of the terms kernel for n_live >= 1 live origins: (nblk, slices), chunk origins per slice
struct OriginSlices {
    int chunk = 0, slices = 0;
};

struct OriginState {
    int max_lag = 0;                // 0 = not configured
    int stride = 0, n = 0, nbins = 0;
    double rmax = 0, dr = 0, inv_dr = 0;
    OriginSizes sz;
    double *d_cur = nullptr, *d_ring = nullptr;
    unsigned long long *d_hist = nullptr, *d_part = nullptr;
    int32_t *d_flag = nullptr, *d_range = nullptr;
    uint64_t *d_sums = nullptr;
    KernelTimer timer;
    int last_live = 0;              // live origins the most recent accumulate visited
    int64_t s = 0;                  // number of the next snapshot of this trajectory
    int64_t snapshots = 0;
    std::vector<int64_t> counts;    // [max_lag + 1] origins that contributed to each lag
};

struct OriginDesc {
    const char *phrase;             // "the van Hove function": "the van Hove function is not configured"
    const char *brief;              // "van Hove": "van Hove launch failed"
    const char *tag;                // "vanhove": ljmd_vanhove_configure, ljmd_vanhove_reset
    const char *limits;             // "VANHOVE": LJMD_VANHOVE_MAX_ORIGINS
    const char *range;              // what LJMD_ERR_RANGE says happened, up to "; the flag stays until ..."
    int components;                 // per particle: 6 = ru xyz, v xyz; 3 = ru xyz
    bool needs_v;
    int max_lag, max_origins;
    size_t max_n;
    int max_bins;                   // 0: no histogram, and configure looks at neither nbins nor rmax
    bool chunk_override;            // ResidentView::vanhove_chunk applies
    // the observable's launches of one accumulate: the gather with ga as it is, and for w.n_live > 0 its terms kernel,
    // the arguments filled from the state, the window and the slices, and the fold with fa as it is
    hipError_t (*launch)(const OriginState &st, const ResidentView &v, const TcfWindow &w, const OriginSlices &p,
                         const ljmdk::OriginGatherArgs &ga, const ljmdk::OriginFoldArgs &fa);
};

OriginSizes origin_sizes(const OriginDesc &d, int n, int max_lag, int stride, int nbins);
// chunk unset: origins per slice by kOriginTargetWorkgroups; set: that many, clamped to [1, min(n_live, kOriginMaxChunk)]
OriginSlices origin_plan_slices(int nblk, int n_live, std::optional<int> chunk = std::nullopt);

int origin_not_configured(const OriginDesc &d, std::string *err, const char *who);
// refuses a multi-device handle and a rank engine of G > 1 itself
int origin_configure(const OriginDesc &d, OriginState *st, std::string *err, const char *who, const ResidentView &v,
                     int32_t max_lag, int32_t origin_stride, int32_t nbins, double rmax);
int origin_accumulate(const OriginDesc &d, OriginState *st, std::string *err, const char *who, const ResidentView &v);
// waits for the device; LJMD_ERR_RANGE while the sticky word is set; hist [max_lag + 1][nbins + 1] or NULL, words
// [2][max_lag + 1][3] or NULL
int origin_fetch(const OriginDesc &d, OriginState *st, std::string *err, const char *who, const ResidentView &v, uint64_t *hist,
                 uint64_t *words, int64_t *counts, int64_t *n_snapshots);
// the two kinds of sums as quotients (tcf_quotient), each [max_lag + 1] or NULL
int origin_read(const OriginDesc &d, OriginState *st, std::string *err, const char *who, const ResidentView &v, uint64_t *hist,
                double *kind0, double *kind1, int64_t *counts, int64_t *n_snapshots);
int origin_reset(const OriginDesc &d, OriginState *st, std::string *err, const char *who, const ResidentView &v);
int origin_profile_read(const OriginDesc &d, OriginState *st, std::string *err, const char *who, const ResidentView &v,
                        double *kernel_ms, int32_t *origins_live);
// ljmd_set_state: the stored origins are dropped and the numbering restarts; histogram, sums and counts stay
void origin_new_trajectory(OriginState *st);
void origin_release(OriginState *st, hipStream_t stream);

}  // namespace ljmdh

namespace ljmdt {

using ljmdh::ResidentView;
using TcfSizes = ljmdh::OriginSizes;
using TcfSlices = ljmdh::OriginSlices;
using TcfState = ljmdh::OriginState;

TcfSizes tcf_sizes(int n, int max_lag, int stride);
TcfSlices tcf_plan_slices(int nblk, int n_live);

int not_configured(std::string *err, const char *who);
int tcf_configure(TcfState *st, std::string *err, const char *who, const ResidentView &v, int32_t max_lag, int32_t origin_stride);
int tcf_accumulate(TcfState *st, std::string *err, const char *who, const ResidentView &v);
int tcf_fetch(TcfState *st, std::string *err, const char *who, const ResidentView &v, uint64_t *words, int64_t *counts,
              int64_t *n_snapshots);
int tcf_read(TcfState *st, std::string *err, const char *who, const ResidentView &v, double *msd, double *vacf, int64_t *counts,
             int64_t *n_snapshots);
int tcf_reset(TcfState *st, std::string *err, const char *who, const ResidentView &v);
int tcf_profile_read(TcfState *st, std::string *err, const char *who, const ResidentView &v, double *kernel_ms,
                     int32_t *origins_live);
void tcf_new_trajectory(TcfState *st);
void tcf_release(TcfState *st, hipStream_t stream);

}  // namespace ljmdt

// The series observables -- the pressure tensor and the heat flux: one state, one core (ljmd_series.cpp), and a constant
// descriptor of each observable (ljmd_stress.cpp, ljmd_heatflux.cpp) that the core is driven by.
namespace ljmdh {

struct SeriesState {
    int max_snapshots = 0;          // 0 = not configured
    int workgroups = 0, blocks = 0; // rows of part / kpart
    uint64_t *d_series = nullptr;   // [max_snapshots][words of a snapshot]
    uint64_t *d_part = nullptr, *d_kpart = nullptr;
    unsigned long long *d_pcount = nullptr, *d_count = nullptr;
    unsigned *d_pflag = nullptr, *d_kflag = nullptr;
    int32_t *d_range = nullptr;
    double *d_bbox = nullptr;       // [T][kRdfBoxStride]
    KernelTimer timer;
    int64_t snapshots = 0;
};

struct SeriesDesc {
    const char *phrase;             // "pressure tensor": "the pressure tensor is not configured"
    const char *tag;                // "stress": ljmd_stress_configure, ljmd_stress_reset
    const char *particle_partials, *particle_flags;     // what a failed allocation calls kpart and kflag
    int words;                      // int64 words of one snapshot
    int pair_components, particle_components;
    int max_snapshots, max_n;
    int kin_block;                  // slots per workgroup of the kinetic kernel
    bool one_rank;                  // a pair term needs both velocities: one-rank engines only
    // the observable's three launches of one accumulate, behind launch_rdf_boxes: fills its pair arguments from the view,
    // the state and the walk, and passes ka and fa on as they are
    hipError_t (*launch)(const SeriesState &st, const ResidentView &v, const ljmdr::RdfWalk &w,
                         const ljmdk::SeriesKineticArgs &ka, const ljmdk::SeriesFoldArgs &fa);
};

int series_not_configured(const SeriesDesc &d, std::string *err, const char *who);
int series_configure(const SeriesDesc &d, SeriesState *st, std::string *err, const char *who, const ResidentView &v,
                     int32_t max_snapshots);
int series_accumulate(const SeriesDesc &d, SeriesState *st, std::string *err, const char *who, const ResidentView &v);
// words [snapshots][d.words], either pointer may be NULL; LJMD_ERR_RANGE while the sticky word is set
int series_fetch(const SeriesDesc &d, SeriesState *st, std::string *err, const char *who, const ResidentView &v, int64_t *words,
                 int64_t *n_snapshots);
// the start of a read in doubles: series_fetch into *w, sized here, when `want`
int series_read_words(const SeriesDesc &d, SeriesState *st, std::string *err, const char *who, const ResidentView &v, bool want,
                      std::vector<int64_t> *w, int64_t *n_snapshots);
int series_reset(const SeriesDesc &d, SeriesState *st, std::string *err, const char *who, const ResidentView &v);
int series_profile_read(const SeriesDesc &d, SeriesState *st, std::string *err, const char *who, const ResidentView &v,
                        int64_t *visited, int64_t *total, double *kernel_ms);
void series_release(const SeriesDesc &d, SeriesState *st, hipStream_t stream);

}  // namespace ljmdh

namespace ljmds {

using ljmdh::ResidentView;
using StressState = ljmdh::SeriesState;

int not_configured(std::string *err, const char *who);
int stress_configure(StressState *st, std::string *err, const char *who, const ResidentView &v, int32_t max_snapshots);
int stress_accumulate(StressState *st, std::string *err, const char *who, const ResidentView &v);
// words [snapshots][kStressWords], either pointer may be NULL; LJMD_ERR_RANGE while the sticky word is set
int stress_fetch(StressState *st, std::string *err, const char *who, const ResidentView &v, int64_t *words, int64_t *n_snapshots);
int stress_read(StressState *st, std::string *err, const char *who, const ResidentView &v, double *p, int64_t *n_snapshots);
int stress_reset(StressState *st, std::string *err, const char *who, const ResidentView &v);
int stress_profile_read(StressState *st, std::string *err, const char *who, const ResidentView &v, int64_t *visited,
                        int64_t *total, double *kernel_ms);
void stress_release(StressState *st, hipStream_t stream);

}  // namespace ljmds

namespace ljmdq {

using ljmdh::ResidentView;
using HeatfluxState = ljmdh::SeriesState;

int not_configured(std::string *err, const char *who);
// refuses a multi-device handle and a rank engine of G > 1 itself
int heatflux_configure(HeatfluxState *st, std::string *err, const char *who, const ResidentView &v, int32_t max_snapshots);
int heatflux_accumulate(HeatfluxState *st, std::string *err, const char *who, const ResidentView &v);
// words [snapshots][kHeatfluxWords], either pointer may be NULL; LJMD_ERR_RANGE while the sticky word is set
int heatflux_fetch(HeatfluxState *st, std::string *err, const char *who, const ResidentView &v, int64_t *words, int64_t *n_snapshots);
// j [snapshots][3], parts [snapshots][3][3], any pointer may be NULL
int heatflux_read(HeatfluxState *st, std::string *err, const char *who, const ResidentView &v, double *j, double *parts,
                  int64_t *n_snapshots);
int heatflux_reset(HeatfluxState *st, std::string *err, const char *who, const ResidentView &v);
int heatflux_profile_read(HeatfluxState *st, std::string *err, const char *who, const ResidentView &v, int64_t *visited,
                          int64_t *total, double *kernel_ms);
void heatflux_release(HeatfluxState *st, hipStream_t stream);

}  // namespace ljmdq

namespace ljmdv {

using ljmdh::ResidentView;
using VhSizes = ljmdh::OriginSizes;
using VhSlices = ljmdh::OriginSlices;
using VanHoveState = ljmdh::OriginState;

VhSizes vanhove_sizes(int n, int max_lag, int stride, int nbins);
// chunk: LJMD_VANHOVE_CHUNK (tests)
VhSlices vanhove_plan_slices(int nblk, int n_live, std::optional<int> chunk = std::nullopt);

int not_configured(std::string *err, const char *who);
int vanhove_configure(VanHoveState *st, std::string *err, const char *who, const ResidentView &v, int32_t max_lag,
                      int32_t origin_stride, int32_t nbins, double rmax);
int vanhove_accumulate(VanHoveState *st, std::string *err, const char *who, const ResidentView &v);
int vanhove_fetch(VanHoveState *st, std::string *err, const char *who, const ResidentView &v, uint64_t *hist, uint64_t *words,
                  int64_t *counts, int64_t *n_snapshots);
int vanhove_read(VanHoveState *st, std::string *err, const char *who, const ResidentView &v, uint64_t *hist, double *r2,
                 double *r4, int64_t *counts, int64_t *n_snapshots);
int vanhove_reset(VanHoveState *st, std::string *err, const char *who, const ResidentView &v);
int vanhove_profile_read(VanHoveState *st, std::string *err, const char *who, const ResidentView &v, double *kernel_ms,
                         int32_t *origins_live);
void vanhove_new_trajectory(VanHoveState *st);
void vanhove_release(VanHoveState *st, hipStream_t stream);

}  // namespace ljmdv

// The density modes (ljmd_rhok.cpp): a series like the pressure tensor's, of n_modes rows of six words per snapshot, with
// a core of its own -- a mode list on the device, no pair part.
namespace ljmdc {

using ljmdh::ResidentView;

struct RhokState {
    int max_snapshots = 0;          // 0 = not configured
    int n_modes = 0, n = 0, T = 0;  // the list's length, and the engine configure saw
    RhokPlan plan;
    uint64_t *d_series = nullptr;   // [max_snapshots][n_modes][kRhokRowWords]
    int32_t *d_modes = nullptr;     // [n_modes][3]
    uint64_t *d_part = nullptr;     // [pchunks][mchunks 64][kRhokRowWords]
    unsigned *d_flag = nullptr;     // [pchunks][mchunks]
    int32_t *d_range = nullptr;
    ljmdh::KernelTimer timer;
    int64_t snapshots = 0;
};

int not_configured(std::string *err, const char *who);
// refuses a multi-device handle and a rank engine of G > 1 itself; copies the list to the device before it returns
int rhok_configure(RhokState *st, std::string *err, const char *who, const ResidentView &v, int32_t n_modes,
                   const int32_t *modes, int32_t max_snapshots);
int rhok_accumulate(RhokState *st, std::string *err, const char *who, const ResidentView &v);
// words [snapshots][n_modes][2][3], either pointer may be NULL; LJMD_ERR_RANGE while the sticky word is set
int rhok_fetch(RhokState *st, std::string *err, const char *who, const ResidentView &v, int64_t *words, int64_t *n_snapshots);
// rho [snapshots][n_modes][2]: fixed_to_double of every integer
int rhok_read(RhokState *st, std::string *err, const char *who, const ResidentView &v, double *rho, int64_t *n_snapshots);
int rhok_reset(RhokState *st, std::string *err, const char *who, const ResidentView &v);
int rhok_profile_read(RhokState *st, std::string *err, const char *who, const ResidentView &v, double *kernel_ms);
void rhok_release(RhokState *st, hipStream_t stream);

// The current modes (ljmd_current.cpp): the density modes' series with eighteen words per mode, on their grid (RhokPlan).
struct CurrentState {
    int max_snapshots = 0;          // 0 = not configured
    int n_modes = 0, n = 0, T = 0;  // the list's length, and the engine configure saw
    RhokPlan plan;
    uint64_t *d_series = nullptr;   // [max_snapshots][n_modes][kCurrentRowWords]
    int32_t *d_modes = nullptr;     // [n_modes][3]
    uint64_t *d_part = nullptr;     // [pchunks][mchunks 64][kCurrentRowWords]
    unsigned *d_flag = nullptr;     // [pchunks][mchunks]
    int32_t *d_range = nullptr;
    ljmdh::KernelTimer timer;
    int64_t snapshots = 0;
};

int current_not_configured(std::string *err, const char *who);
// refuses a multi-device handle and a rank engine of G > 1 itself; copies the list to the device before it returns
int current_configure(CurrentState *st, std::string *err, const char *who, const ResidentView &v, int32_t n_modes,
                      const int32_t *modes, int32_t max_snapshots);
int current_accumulate(CurrentState *st, std::string *err, const char *who, const ResidentView &v);
// words [snapshots][n_modes][3][2][3], either pointer may be NULL; LJMD_ERR_RANGE while the sticky word is set
int current_fetch(CurrentState *st, std::string *err, const char *who, const ResidentView &v, int64_t *words,
                  int64_t *n_snapshots);
// j [snapshots][n_modes][3][2]: fixed_to_double of every integer
int current_read(CurrentState *st, std::string *err, const char *who, const ResidentView &v, double *j, int64_t *n_snapshots);
int current_reset(CurrentState *st, std::string *err, const char *who, const ResidentView &v);
int current_profile_read(CurrentState *st, std::string *err, const char *who, const ResidentView &v, double *kernel_ms);
void current_release(CurrentState *st, hipStream_t stream);

}  // namespace ljmdc
#endif
