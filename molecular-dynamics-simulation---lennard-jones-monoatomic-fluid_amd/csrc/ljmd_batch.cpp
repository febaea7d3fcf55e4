// ljmd_batch.cpp -- host side of the batch engine (include/ljmd.h: ljmd_batch_*): B independent replicas on one
// device, each with its own (n, L, dt, rc) (ljmd_batch_create: all the same), stepped by one kernel (ljmd_batch.hip)
// with one workgroup per replica.  Handle lifecycle, guards, device state, launch planning per kernel class and the
// combination of the per-replica step records, in the fp64 mode and in the reproducible mode (ljmd_batch_fixed.hip:
// exact integer records, a sticky range flag per replica), the g(r) accumulation (ljmd_batch_rdf.hip) and the MSD / VACF
// accumulation (ljmd_batch_tcf.hip).
#include "ljmd_batch.h"
#include "ljmd_common.h"
#include "ljmd_internal.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

using namespace ljmdb;
using ljmdh::fail;

namespace {

// one replica's parameters and derived constants (host side)
struct BatchRep : ljmdh::SimParams {
    int n = 0;
};

// the replicas of one kernel class: entries [first, first + count) of the replica table, launched chunk replicas and
// steps_per_launch steps at a time (launch_shape of n_max, the group's largest n)
struct BatchGroup {
    size_t first = 0, count = 0;
    int n_max = 0;
    size_t chunk = 0;
    int steps_per_launch = 0;
    size_t rdf_chunk = 0;             // replicas per g(r) launch: launch_shape's pair bound of the fp64 mode, one step
    hipStream_t stream = nullptr;     // own stream when the handle runs its groups concurrently, else the handle's
    hipEvent_t done = nullptr;
};

}  // namespace

struct ljmd_batch {
    size_t B = 0;
    size_t total = 0;                 // offsets[B]: elements of one plane
    int device = 0;
    std::vector<BatchRep> rep;        // [B], replica order
    std::vector<int64_t> offsets;     // [B + 1]
    std::vector<BatchGroup> groups;   // by kernel class, ascending
    bool concurrent = false;          // groups on streams of their own, joined before the records are fetched
    int mode = LJMD_PRECISION_FP64;   // or LJMD_PRECISION_FP64_REPRODUCIBLE (ljmd_batch_set_precision)
    bool tail_on = true;
    bool have_state = false, have_accel = false;
    bool poisoned = false;            // a launch failed half-way: LJMD_ERR_STATE until ljmd_batch_set_state
    hipStream_t stream = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    hipEvent_t fork = nullptr;
    BatchReplica *d_table = nullptr;  // [B], the groups' entries one after another
    double *d_state = nullptr;        // [12][offsets[B]]
    double *d_rec = nullptr;          // [samples][B][rec_words]: doubles, or int64 words in the reproducible mode
    size_t rec_cap = 0;               // 8-byte words the record buffer holds (>= B * kExactWords)
    std::vector<double> h_rec;
    int32_t *d_range = nullptr;       // [B] reproducible mode: sticky range flags, cleared by ljmd_batch_set_state
    std::vector<int32_t> h_range;
    double last_ms = 0.0;             // kernel time of the last ljmd_batch_steps call
    int32_t last_launches = 0;
    // g(r) accumulation (ljmd_batch_rdf_*): off while rdf_nbins == 0
    int32_t rdf_nbins = 0, rdf_every = 0;
    int64_t rdf_snapshots = 0;
    unsigned long long *d_rdf_hist = nullptr;   // [B][rdf_nbins]
    BatchRdfReplica *d_rdf_table = nullptr;     // [B], replica order
    // MSD / VACF accumulation (ljmd_batch_tcf_*): off while tcf_max_lag == 0
    int32_t tcf_max_lag = 0, tcf_stride = 1, tcf_every = 0, tcf_slots = 0;
    int64_t tcf_s = 0;                // number of the next snapshot of this trajectory (0 after ljmd_batch_set_state)
    int64_t tcf_snapshots = 0;        // snapshots since configure / reset, over all trajectories
    std::vector<int64_t> tcf_counts;  // [max_lag + 1] origins that contributed to each lag: the same for all replicas
    uint64_t *d_tcf_sums = nullptr;   // [B][2][max_lag + 1][3] signed 192-bit
    int32_t *d_tcf_range = nullptr;   // [B] sticky until ljmd_batch_tcf_reset
    double *d_tcf_ring = nullptr;     // [slots][6][offsets[B]]: ru and v of the stored origins
    std::string err;
};

namespace {

// pair evaluations per launch: ~15 ms at the estimated 1.3e12 ordered pairs/s of one MI355X (27 fp64 VALU ops per pair,
// DESIGN.md 3.1), so that a launch stays well under 100 ms even at a third of that rate
constexpr double kLaunchPairs = 2e10;
constexpr double kMinParallel = 256;  // below one replica per CU a launch does not get shorter
// ... and a bound for a workgroup that runs alone on its CU, where latency, not throughput, sets the pace: one pass of a
// wave over j costs ~30 dependent fp64 instructions, at most ~100 ns; 2e5 iterations of it per launch = <= 20 ms
constexpr double kLaunchIterations = 2e5;
// The reproducible mode (ljmd_batch_fixed.hip): ~230 VALU instructions per pair against ~34 gave the
// starting values 3e9 / 3e4, whose launches measured 12.6-18.9 ms on one MI355X; raised by 1.2 to bring every class
// into the 16-22 ms of the fp64 launches.  Measured full launches of these values (tools/batch_reproducible_rate.py,
// profiles/batch_reproducible_rate.txt), n (B): steps per launch, kernel time:
//   108 (4096): 75, 20.9 ms    500 (1024): 14, 16.9 ms    4000 (256): 1, 18.6 ms
//   108 (1):   333, 16.7 ms    500 (1):    56, 19.2 ms    4000 (1):   1, 18.8 ms
// = 1.7-2.2e11 ordered pairs/s and 0.47-1.17 us per pass over j.  From n = 3424 on one step of 256 replicas is already
// more than kFixedLaunchPairs; a launch cannot hold less than one step, and fewer replicas than CUs do not shorten it.
constexpr double kFixedLaunchPairs = 3.6e9;
constexpr double kFixedLaunchIterations = 3.6e4;

// the exact record's layout and flag bits are the kernels' (ljmd_internal.h); the range flag that counts is the sticky
// word, not the record's
using ljmdk::kExactWords;
using ljmdk::kFlagNoEnergy;
using ljmdk::kFlagNoKinetic;
static_assert(kExactWords == LJMD_EXACT_PARTIAL_WORDS, "exact record layout out of sync with include/ljmd.h");
static_assert(kBatchTcfMaxLag == LJMD_BATCH_TCF_MAX_LAG && kBatchTcfMaxOrigins == LJMD_BATCH_TCF_MAX_ORIGINS,
              "MSD / VACF limits out of sync with include/ljmd.h");

bool reproducible(const ljmd_batch *h) { return h->mode == LJMD_PRECISION_FP64_REPRODUCIBLE; }
size_t rec_words(const ljmd_batch *h) { return reproducible(h) ? kExactWords : kBatchRecWords; }

double *plane(ljmd_batch *h, int which, int axis) { return h->d_state + ((size_t)which * 3 + axis) * h->total; }

BatchArgs base_args(ljmd_batch *h, int mode)
{
    BatchArgs a{};
    a.state = h->d_state;
    a.rec = h->d_rec;
    a.rep = h->d_table;
    a.B = h->B;
    a.plane = h->total;
    a.mode = mode;
    return a;
}

// replicas per launch and steps per launch of `count` replicas of at most n particles, from the
// n^2 * steps * max(replicas, CUs) estimate
void launch_shape(int n, size_t count, bool fixed, size_t *chunk, int *steps_per_launch)
{
    const double pairs = fixed ? kFixedLaunchPairs : kLaunchPairs;
    const double iterations = fixed ? kFixedLaunchIterations : kLaunchIterations;
    const double n2 = (double)n * n;
    const double c = std::max(kMinParallel, std::floor(pairs / n2));
    *chunk = std::min(count, (size_t)std::min(c, 2147483647.0));
    const double s = std::floor(pairs / (n2 * std::max(kMinParallel, (double)*chunk)));
    // passes over j per step: ljmd_batch.hip works two own particles per pass (KG), ljmd_batch_fixed.hip one
    const int passes = fixed ? batch_k(n) : (batch_k(n) + 1) / 2;
    const double s_latency = std::floor(iterations / ((double)n * passes));
    *steps_per_launch = (int)std::max(1.0, std::min({s, s_latency, (double)LJMD_MAX_PENDING_STEPS}));
}

BatchRep derive(int n, double box_length, double dt, double rc)
{
    BatchRep r;
    static_cast<ljmdh::SimParams &>(r) = ljmdh::derive_params(n, box_length, dt, rc);
    r.n = n;
    return r;
}

// room for `samples` records of the handle's mode (at least one of either mode)
int ensure_records(ljmd_batch *h, size_t samples)
{
    const size_t words = std::max(samples * h->B * rec_words(h), h->B * (size_t)kExactWords);
    if (words <= h->rec_cap) return LJMD_OK;
    if (h->d_rec) (void)hipFree(h->d_rec);
    h->d_rec = nullptr;
    h->rec_cap = 0;
    const size_t bytes = words * sizeof(double);
    if (hipMalloc(&h->d_rec, bytes) != hipSuccess) {
        h->d_rec = nullptr;
        return fail(h, LJMD_ERR_ALLOC, "ljmd_batch: cannot allocate %zu bytes of step records", bytes);
    }
    h->rec_cap = words;
    return LJMD_OK;
}

// copies `samples` records to the host; the handle is poisoned when the kernels behind them failed.  Reproducible
// mode: the range flags come along, and a set flag -- of a sampled or an unsampled step -- fails the call with
// LJMD_ERR_RANGE, names the lowest such replica and poisons the handle
int fetch_records(ljmd_batch *h, size_t samples, const char *who)
{
    h->h_rec.resize(samples * h->B * rec_words(h));
    hipError_t e = hipMemcpyAsync(h->h_rec.data(), h->d_rec, h->h_rec.size() * sizeof(double), hipMemcpyDeviceToHost,
                                  h->stream);
    if (e == hipSuccess && reproducible(h))
        e = hipMemcpyAsync(h->h_range.data(), h->d_range, h->B * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream);
    const hipError_t s = e == hipSuccess ? hipStreamSynchronize(h->stream) : e;
    if (s != hipSuccess) {
        h->poisoned = true;
        return fail(h, LJMD_ERR_HIP, "ljmd_batch: kernel or copy failed: %s; the handle is poisoned until "
                                      "ljmd_batch_set_state", hipGetErrorString(s));
    }
    if (reproducible(h))
        for (size_t b = 0; b < h->B; ++b)
            if (h->h_range[b] != 0) {
                h->poisoned = true;
                return fail(h, LJMD_ERR_RANGE, "%s: reproducible mode: replica %zu: a pair or velocity term was not "
                                               "finite or |term| >= 2^40 (particles closer than about 0.12 sigma?); "
                                               "the handle is poisoned until ljmd_batch_set_state", who, b);
            }
    return LJMD_OK;
}

// as combine_one (ljmd_records.cpp) for replica b's record: the kernel already halved the ordered-pair sums.
// Reproducible mode: as combine_exact for the replica's one exact record (the words of r are int64)
void combine(const ljmd_batch *h, size_t b, const double *r, double *epot, double *ekin, double *d_epot, double *dd_epot)
{
    const BatchRep &p = h->rep[b];
    const double te = h->tail_on ? p.tail_e : 0.0, td = h->tail_on ? p.tail_d : 0.0, tdd = h->tail_on ? p.tail_dd : 0.0;
    if (!reproducible(h)) {
        ljmdh::scalars_from_sums(r[0], r[1], r[2], r[3], r[4], te, td, tdd, epot, ekin, d_epot, dd_epot);
        return;
    }
    uint64_t sum[5][3];
    int64_t flags;
    std::memcpy(sum, r, sizeof sum);
    std::memcpy(&flags, r + 15, sizeof flags);
    ljmdh::scalars_from_exact_sums(sum, te, td, tdd, !(flags & kFlagNoEnergy), !(flags & kFlagNoKinetic), epot, ekin,
                                   d_epot, dd_epot);
}

int upload(ljmd_batch *h, int which, int axis, const double *src)
{
    LJMD_HIP(h, hipMemcpyAsync(plane(h, which, axis), src, h->total * sizeof(double), hipMemcpyHostToDevice,
                                h->stream));
    return LJMD_OK;
}

// the g(r) launches of group g on stream s: the positions resident now, chunks of at most rdf_chunk replicas
int enqueue_rdf(ljmd_batch *h, const BatchGroup &g, hipStream_t s, int32_t *count, const char *who)
{
    BatchRdfArgs ra{};
    ra.r = plane(h, LJMD_R, 0);
    ra.rep = h->d_table;
    ra.rdf = h->d_rdf_table;
    ra.hist = h->d_rdf_hist;
    ra.plane = h->total;
    ra.nbins = h->rdf_nbins;
    for (size_t c0 = 0; c0 < g.count; c0 += g.rdf_chunk) {
        ra.g0 = (int)(g.first + c0);
        const hipError_t e = launch_batch_rdf(ra, g.n_max, (int)std::min(g.rdf_chunk, g.count - c0), s);
        ++*count;
        if (e != hipSuccess) {
            h->poisoned = true;
            return fail(h, LJMD_ERR_HIP, "%s: g(r) launch failed: %s; the handle is poisoned until ljmd_batch_set_state",
                         who, hipGetErrorString(e));
        }
    }
    return LJMD_OK;
}

// The live origins of snapshot s: the multiples t0 of the stride with 1 <= s - t0 <= max_lag (BatchTcfArgs)
struct TcfLive {
    int n_live = 0, lag_first = 0, slot_first = 0, store_slot = -1;
};
TcfLive tcf_live(const ljmd_batch *h, int64_t s)
{
    const int64_t stride = h->tcf_stride, lo = std::max<int64_t>(0, s - h->tcf_max_lag);
    const int64_t first = (lo + stride - 1) / stride * stride, last = s >= 1 ? (s - 1) / stride * stride : -1;
    TcfLive l;
    if (last >= first) {
        l.n_live = (int)((last - first) / stride) + 1;
        l.lag_first = (int)(s - first);
        l.slot_first = (int)(first / stride % h->tcf_slots);
    }
    if (s % stride == 0) l.store_slot = (int)(s / stride % h->tcf_slots);
    return l;
}

// the MSD / VACF launch of group g on stream s_: the resident ru and v as snapshot number snap -- one launch per group
int enqueue_tcf(ljmd_batch *h, const BatchGroup &g, hipStream_t s_, int64_t snap, int32_t *count, const char *who)
{
    const TcfLive l = tcf_live(h, snap);
    if (l.n_live == 0 && l.store_slot < 0) return LJMD_OK;
    BatchTcfArgs ta{};
    ta.state = h->d_state;
    ta.ring = h->d_tcf_ring;
    ta.sums = h->d_tcf_sums;
    ta.range = h->d_tcf_range;
    ta.rep = h->d_table;
    ta.plane = h->total;
    ta.g0 = (int)g.first;
    ta.max_lag = h->tcf_max_lag;
    ta.stride = h->tcf_stride;
    ta.slots = h->tcf_slots;
    ta.n_live = l.n_live;
    ta.lag_first = l.lag_first;
    ta.slot_first = l.slot_first;
    ta.store_slot = l.store_slot;
    const hipError_t e = launch_batch_tcf(ta, g.n_max, (int)g.count, s_);
    ++*count;
    if (e != hipSuccess) {
        h->poisoned = true;
        return fail(h, LJMD_ERR_HIP, "%s: MSD / VACF launch failed: %s; the handle is poisoned until ljmd_batch_set_state",
                     who, hipGetErrorString(e));
    }
    return LJMD_OK;
}

// the host's share of one snapshot, once every group's launch is enqueued: the counts and the numbering
void tcf_advance(ljmd_batch *h)
{
    const TcfLive l = tcf_live(h, h->tcf_s);
    for (int e = 0; e < l.n_live; ++e) {
        const int lag = l.lag_first - e * h->tcf_stride;
        ++h->tcf_counts[(size_t)lag];
        if (lag == 1) ++h->tcf_counts[0];
    }
    ++h->tcf_s;
    ++h->tcf_snapshots;
}

// one pass of the kernel over every replica in `mode`: nsteps steps (kModeSteps) or one evaluation.  Group by group,
// launches of at most chunk replicas and steps_per_launch steps, in the order steps-outer, replicas-inner.  With
// concurrent groups every group runs on its own stream between a fork from and a join into the handle's stream, so
// what the handle's stream does next (the record copy) follows all of them.  A failed launch poisons the handle.
// rdf_every > 0 (kModeSteps only): a launch ends at the steps rdf_every, 2 rdf_every, ..., and the group's g(r)
// launches follow it on the same stream; 0 is the launch sequence without g(r).  tcf_every > 0: the same for the
// MSD / VACF snapshots, numbered on from h->tcf_s (the caller advances the numbering afterwards).
int run_groups(ljmd_batch *h, BatchArgs a, int nsteps, int rdf_every, int tcf_every, int32_t *launches, const char *who)
{
    if (h->concurrent) {
        LJMD_HIP(h, hipEventRecord(h->fork, h->stream));
        for (const BatchGroup &g : h->groups) LJMD_HIP(h, hipStreamWaitEvent(g.stream, h->fork, 0));
    }
    const bool steps = a.mode == kModeSteps;
    int32_t count = 0;
    for (const BatchGroup &g : h->groups) {
        hipStream_t s = h->concurrent ? g.stream : h->stream;
        const int spl = steps ? g.steps_per_launch : 1;
        for (int s0 = 0, len = 0; s0 < (steps ? nsteps : 1); s0 += len) {
            len = std::min(spl, (steps ? nsteps : 1) - s0);
            if (rdf_every > 0) len = std::min(len, rdf_every - s0 % rdf_every);
            if (tcf_every > 0) len = std::min(len, tcf_every - s0 % tcf_every);
            a.step0 = s0;
            a.nsteps = steps ? len : 0;
            for (size_t c0 = 0; c0 < g.count; c0 += g.chunk) {
                a.g0 = (int)(g.first + c0);
                const int blocks = (int)std::min(g.chunk, g.count - c0);
                const hipError_t e = reproducible(h)
                    ? launch_batch_fixed(BatchFixedArgs{a, reinterpret_cast<int64_t *>(h->d_rec), h->d_range}, g.n_max,
                                         blocks, s)
                    : launch_batch(a, g.n_max, blocks, s);
                ++count;
                if (e != hipSuccess) {
                    h->poisoned = true;
                    if (steps)
                        return fail(h, LJMD_ERR_HIP, "%s: launch at step %d failed: %s; the handle is poisoned until "
                                                      "ljmd_batch_set_state", who, s0, hipGetErrorString(e));
                    return fail(h, LJMD_ERR_HIP, "%s: launch failed: %s", who, hipGetErrorString(e));
                }
            }
            if (rdf_every > 0 && (s0 + len) % rdf_every == 0) {
                const int rc_ = enqueue_rdf(h, g, s, &count, who);
                if (rc_ != LJMD_OK) return rc_;
            }
            if (tcf_every > 0 && (s0 + len) % tcf_every == 0) {
                const int rc_ = enqueue_tcf(h, g, s, h->tcf_s + (s0 + len) / tcf_every - 1, &count, who);
                if (rc_ != LJMD_OK) return rc_;
            }
        }
        if (h->concurrent) {
            LJMD_HIP(h, hipEventRecord(g.done, s));
            LJMD_HIP(h, hipStreamWaitEvent(h->stream, g.done, 0));
        }
    }
    if (launches) *launches = count;
    return LJMD_OK;
}

// releases the g(r) buffers after what may still use them
void rdf_release(ljmd_batch *h)
{
    if (h->stream && (h->d_rdf_hist || h->d_rdf_table)) (void)hipStreamSynchronize(h->stream);
    if (h->d_rdf_hist) (void)hipFree(h->d_rdf_hist);
    if (h->d_rdf_table) (void)hipFree(h->d_rdf_table);
    h->d_rdf_hist = nullptr;
    h->d_rdf_table = nullptr;
    h->rdf_nbins = 0;
    h->rdf_every = 0;
    h->rdf_snapshots = 0;
}

// releases the MSD / VACF buffers after what may still use them
void tcf_release(ljmd_batch *h)
{
    if (h->stream && (h->d_tcf_sums || h->d_tcf_range || h->d_tcf_ring)) (void)hipStreamSynchronize(h->stream);
    if (h->d_tcf_sums) (void)hipFree(h->d_tcf_sums);
    if (h->d_tcf_range) (void)hipFree(h->d_tcf_range);
    if (h->d_tcf_ring) (void)hipFree(h->d_tcf_ring);
    h->d_tcf_sums = nullptr;
    h->d_tcf_range = nullptr;
    h->d_tcf_ring = nullptr;
    h->tcf_max_lag = 0;
    h->tcf_stride = 1;
    h->tcf_every = 0;
    h->tcf_slots = 0;
    h->tcf_s = 0;
    h->tcf_snapshots = 0;
    h->tcf_counts.clear();
}

size_t tcf_sum_words(const ljmd_batch *h) { return h->B * 2 * ((size_t)h->tcf_max_lag + 1) * 3; }

// the guards shared by ljmd_batch_tcf_read and ljmd_batch_tcf_read_exact, then the device's sums in h_words: waits for
// the device; a set range word fails the call and names the lowest such replica
int tcf_fetch(ljmd_batch *h, std::vector<uint64_t> *h_words, const char *who)
{
    if (!h) return fail(nullptr, LJMD_ERR_INVALID_ARG, "%s: NULL handle", who);
    if (h->tcf_max_lag == 0) return fail(h, LJMD_ERR_STATE, "%s: call ljmd_batch_tcf_configure first", who);
    LJMD_HIP(h, hipSetDevice(h->device));
    std::vector<int32_t> range;
    try {
        range.resize(h->B);
        if (h_words) h_words->resize(tcf_sum_words(h));
    } catch (const std::bad_alloc &) {
        return fail(h, LJMD_ERR_ALLOC, "%s: out of host memory", who);
    }
    hipError_t e = hipMemcpyAsync(range.data(), h->d_tcf_range, h->B * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess && h_words)
        e = hipMemcpyAsync(h_words->data(), h->d_tcf_sums, h_words->size() * sizeof(uint64_t), hipMemcpyDeviceToHost,
                           h->stream);
    const hipError_t s = hipStreamSynchronize(h->stream);
    if (e != hipSuccess || s != hipSuccess) {
        h->poisoned = true;
        return fail(h, LJMD_ERR_HIP, "%s: kernel or copy failed: %s; the handle is poisoned until ljmd_batch_set_state",
                     who, hipGetErrorString(e != hipSuccess ? e : s));
    }
    for (size_t b = 0; b < h->B; ++b)
        if (range[b] != 0)
            return fail(h, LJMD_ERR_RANGE, "%s: replica %zu: an MSD or VACF term was not finite or |term| >= 2^40 and "
                                           "entered as 0; the flag stays until ljmd_batch_tcf_reset", who, b);
    return LJMD_OK;
}

// the handle from its replicas' parameters, after the guards and the probe: groups, stream(s), device memory
int create_handle(ljmd_batch_t **out, std::vector<BatchRep> &&reps, int32_t device, const char *who)
{
    ljmd_batch *h = new (std::nothrow) ljmd_batch;
    if (!h) return fail(nullptr, LJMD_ERR_ALLOC, "%s: out of host memory", who);
    auto body = [&]() -> int {
        h->B = reps.size();
        h->device = device;
        std::vector<BatchReplica> table;
        try {
            h->rep = std::move(reps);
            h->offsets.resize(h->B + 1);
            table.reserve(h->B);
        } catch (const std::bad_alloc &) {
            return fail(h, LJMD_ERR_ALLOC, "%s: out of host memory", who);
        }
        h->offsets[0] = 0;
        for (size_t b = 0; b < h->B; ++b) h->offsets[b + 1] = h->offsets[b] + h->rep[b].n;
        h->total = (size_t)h->offsets[h->B];
        // the replica table, grouped by kernel class; replica order inside a group
        for (int c = 0; c < kBatchClasses; ++c) {
            BatchGroup g;
            g.first = table.size();
            for (size_t b = 0; b < h->B; ++b) {
                const BatchRep &p = h->rep[b];
                if (batch_class(p.n) != c) continue;
                BatchReplica e{};
                e.off = (size_t)h->offsets[b];
                e.b = (int)b;
                e.n = p.n;
                e.threads = batch_threads(p.n);
                e.L = p.L;
                e.invL = p.invL;
                e.rc2 = p.rc2;
                e.dt = p.dt;
                e.dt_half = p.dt_half;
                e.dt_sq_half = p.dt_sq_half;
                table.push_back(e);
                g.n_max = std::max(g.n_max, p.n);
            }
            g.count = table.size() - g.first;
            if (g.count == 0) continue;
            launch_shape(g.n_max, g.count, reproducible(h), &g.chunk, &g.steps_per_launch);
            int one_step = 0;
            launch_shape(g.n_max, g.count, false, &g.rdf_chunk, &one_step);
            h->groups.push_back(g);
        }
        // several groups run concurrently unless LJMD_BATCH_GROUP_STREAMS=0 (one after another on the handle's stream)
        h->concurrent = h->groups.size() > 1 && ljmdh::read_knobs().batch_group_streams;
        if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess ||
            hipEventCreate(&h->ev[0]) != hipSuccess || hipEventCreate(&h->ev[1]) != hipSuccess)
            return fail(h, LJMD_ERR_HIP, "%s: cannot create the stream on device %d", who, device);
        if (h->concurrent) {
            bool ok = hipEventCreateWithFlags(&h->fork, hipEventDisableTiming) == hipSuccess;
            for (BatchGroup &g : h->groups)
                ok = ok && hipStreamCreateWithFlags(&g.stream, hipStreamNonBlocking) == hipSuccess &&
                     hipEventCreateWithFlags(&g.done, hipEventDisableTiming) == hipSuccess;
            if (!ok) return fail(h, LJMD_ERR_HIP, "%s: cannot create the group streams on device %d", who, device);
        }
        const size_t bytes = 12 * h->total * sizeof(double);
        if (hipMalloc(&h->d_state, bytes) != hipSuccess) {
            h->d_state = nullptr;
            return fail(h, LJMD_ERR_ALLOC, "%s: cannot allocate %zu bytes of replica state", who, bytes);
        }
        const size_t tbytes = h->B * sizeof(BatchReplica);
        if (hipMalloc(&h->d_table, tbytes) != hipSuccess) {
            h->d_table = nullptr;
            return fail(h, LJMD_ERR_ALLOC, "%s: cannot allocate %zu bytes of the replica table", who, tbytes);
        }
        if (hipMemcpyAsync(h->d_table, table.data(), tbytes, hipMemcpyHostToDevice, h->stream) != hipSuccess ||
            hipStreamSynchronize(h->stream) != hipSuccess)
            return fail(h, LJMD_ERR_HIP, "%s: cannot upload the replica table", who);
        try {
            h->h_range.assign(h->B, 0);
        } catch (const std::bad_alloc &) {
            return fail(h, LJMD_ERR_ALLOC, "%s: out of host memory", who);
        }
        if (hipMalloc(&h->d_range, h->B * sizeof(int32_t)) != hipSuccess) {
            h->d_range = nullptr;
            return fail(h, LJMD_ERR_ALLOC, "%s: cannot allocate %zu bytes of range flags", who, h->B * sizeof(int32_t));
        }
        if (hipMemsetAsync(h->d_range, 0, h->B * sizeof(int32_t), h->stream) != hipSuccess ||
            hipStreamSynchronize(h->stream) != hipSuccess)
            return fail(h, LJMD_ERR_HIP, "%s: cannot clear the range flags", who);
        return ensure_records(h, 1);
    };
    const int rc_ = body();
    if (rc_ != LJMD_OK) {                  // one release on failure; the message outlives the handle
        const std::string msg = h->err;
        ljmd_batch_destroy(h);
        ljmdh::g_last_error = msg;
        return rc_;
    }
    *out = h;
    return LJMD_OK;
}

}  // namespace

extern "C" {

const char *ljmd_batch_last_error(const ljmd_batch_t *h) { return h ? h->err.c_str() : ljmdh::g_last_error.c_str(); }

int ljmd_batch_create(ljmd_batch_t **out, int32_t n_replicas, int32_t n, double box_length, double dt, double rc,
                      int32_t precision_mode, int32_t device)
{
    if (!out) return fail(nullptr, LJMD_ERR_INVALID_ARG, "ljmd_batch_create: out is NULL");
    *out = nullptr;
    // the guards of ljmd_create (md_types.f90:143-161), then the batch engine's own
    LJMD_TRY(ljmdh::check_sim_params("ljmd_batch_create", n, box_length, dt, rc));
    if (n_replicas < 1) return fail(nullptr, LJMD_ERR_INVALID_ARG, "ljmd_batch_create: n_replicas must be >= 1");
    if (n > LJMD_BATCH_MAX_N)
        return fail(nullptr, LJMD_ERR_INVALID_ARG, "ljmd_batch_create: n must be <= LJMD_BATCH_MAX_N (%d)",
                     LJMD_BATCH_MAX_N);
    if (precision_mode != LJMD_PRECISION_FP64)
        return fail(nullptr, LJMD_ERR_INVALID_ARG, "ljmd_batch_create: precision_mode %d not available for batches "
                                                    "(LJMD_PRECISION_FP64 only)", precision_mode);
    if (!(rc <= (1.0 - 1e-9) * 0.5 * box_length))
        return fail(nullptr, LJMD_ERR_INVALID_ARG, "ljmd_batch_create: rc must be <= (1 - 1e-9) L/2 (fast-path "
                                                    "precondition; batches have no generic kernel)");
    const int rc_ = ljmdh::probe_device(device, "ljmd_batch_create");
    if (rc_ != LJMD_OK) return rc_;
    std::vector<BatchRep> reps;
    try {
        reps.assign((size_t)n_replicas, derive(n, box_length, dt, rc));
    } catch (const std::bad_alloc &) {
        return fail(nullptr, LJMD_ERR_ALLOC, "ljmd_batch_create: out of host memory");
    }
    return create_handle(out, std::move(reps), device, "ljmd_batch_create");
}

int ljmd_batch_create_per_replica(ljmd_batch_t **out, int32_t n_replicas, const int32_t *n, const double *box_length,
                                  const double *dt, const double *rc, int32_t precision_mode, int32_t device)
{
    static const char *who = "ljmd_batch_create_per_replica";
    if (!out) return fail(nullptr, LJMD_ERR_INVALID_ARG, "%s: out is NULL", who);
    *out = nullptr;
    if (n_replicas < 1) return fail(nullptr, LJMD_ERR_INVALID_ARG, "%s: n_replicas must be >= 1", who);
    if (!n || !box_length || !dt || !rc)
        return fail(nullptr, LJMD_ERR_INVALID_ARG, "%s: n, box_length, dt and rc must not be NULL", who);
    if (precision_mode != LJMD_PRECISION_FP64)
        return fail(nullptr, LJMD_ERR_INVALID_ARG, "%s: precision_mode %d not available for batches "
                                                    "(LJMD_PRECISION_FP64 only)", who, precision_mode);
    // every replica passes the guards of ljmd_batch_create
    int64_t total = 0;
    for (int32_t b = 0; b < n_replicas; ++b) {
        const double L = box_length[b];
        if (n[b] <= 0 || n[b] > LJMD_BATCH_MAX_N)
            return fail(nullptr, LJMD_ERR_INVALID_ARG, "%s: replica %d: n = %d outside 1..LJMD_BATCH_MAX_N (%d)", who,
                         b, n[b], LJMD_BATCH_MAX_N);
        if (!(L > 0.0)) return fail(nullptr, LJMD_ERR_INVALID_ARG, "%s: replica %d: box_length must be > 0", who, b);
        if (!(dt[b] > 0.0)) return fail(nullptr, LJMD_ERR_INVALID_ARG, "%s: replica %d: dt must be > 0", who, b);
        if (!(rc[b] > 0.0)) return fail(nullptr, LJMD_ERR_INVALID_ARG, "%s: replica %d: rc must be > 0", who, b);
        if (!(rc[b] <= (1.0 - 1e-9) * 0.5 * L))
            return fail(nullptr, LJMD_ERR_INVALID_ARG, "%s: replica %d: rc must be <= (1 - 1e-9) L/2 (fast-path "
                                                        "precondition; batches have no generic kernel)", who, b);
        total += n[b];
    }
    if (total >= ((int64_t)1 << 31))
        return fail(nullptr, LJMD_ERR_INVALID_ARG, "%s: %lld particles in all; the sum of n must be < 2^31", who,
                     (long long)total);
    const int rc_ = ljmdh::probe_device(device, who);
    if (rc_ != LJMD_OK) return rc_;
    std::vector<BatchRep> reps;
    try {
        reps.reserve((size_t)n_replicas);
        for (int32_t b = 0; b < n_replicas; ++b) reps.push_back(derive(n[b], box_length[b], dt[b], rc[b]));
    } catch (const std::bad_alloc &) {
        return fail(nullptr, LJMD_ERR_ALLOC, "%s: out of host memory", who);
    }
    return create_handle(out, std::move(reps), device, who);
}

int ljmd_batch_offsets(const ljmd_batch_t *h, int64_t *offsets)
{
    if (!h || !offsets) return fail(h, LJMD_ERR_INVALID_ARG, "ljmd_batch_offsets: NULL argument");
    std::copy(h->offsets.begin(), h->offsets.end(), offsets);
    return LJMD_OK;
}

void ljmd_batch_destroy(ljmd_batch_t *h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (h->d_state) (void)hipFree(h->d_state);
    for (const BatchGroup &g : h->groups)
        if (g.stream) (void)hipStreamSynchronize(g.stream);
    if (h->d_rec) (void)hipFree(h->d_rec);
    if (h->d_table) (void)hipFree(h->d_table);
    if (h->d_range) (void)hipFree(h->d_range);
    rdf_release(h);
    tcf_release(h);
    for (hipEvent_t e : h->ev)
        if (e) (void)hipEventDestroy(e);
    if (h->fork) (void)hipEventDestroy(h->fork);
    for (const BatchGroup &g : h->groups) {
        if (g.done) (void)hipEventDestroy(g.done);
        if (g.stream) (void)hipStreamDestroy(g.stream);
    }
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

int ljmd_batch_set_state(ljmd_batch_t *h, const double *rx, const double *ry, const double *rz, const double *vx,
                         const double *vy, const double *vz)
{
    if (!h) return fail(nullptr, LJMD_ERR_INVALID_ARG, "ljmd_batch_set_state: NULL handle");
    if (!rx || !ry || !rz || !vx || !vy || !vz) return fail(h, LJMD_ERR_INVALID_ARG, "ljmd_batch_set_state: NULL array");
    // fast-path precondition (a), ljmd_kernels.hip: per replica and axis, finite coordinates spanning < 2.4 L_b
    const double *src[3] = {rx, ry, rz};
    for (size_t b = 0; b < h->B; ++b)
        for (int ax = 0; ax < 3; ++ax) {
            const double *p = src[ax] + h->offsets[b];
            double lo = INFINITY, hi = -INFINITY;
            for (int i = 0; i < h->rep[b].n; ++i) {
                lo = std::min(lo, p[i]);
                hi = std::max(hi, p[i]);
                if (!std::isfinite(p[i]))
                    return fail(h, LJMD_ERR_INVALID_ARG, "ljmd_batch_set_state: replica %zu has a non-finite position", b);
            }
            if (!(hi - lo < 2.4 * h->rep[b].L))
                return fail(h, LJMD_ERR_INVALID_ARG, "ljmd_batch_set_state: replica %zu spans >= 2.4 L along axis %d "
                                                      "(wrap the positions first)", b, ax);
        }
    LJMD_HIP(h, hipSetDevice(h->device));
    if (h->poisoned) {
        (void)hipStreamSynchronize(h->stream);   // drain what a failed call left behind
        for (const BatchGroup &g : h->groups)
            if (g.stream) (void)hipStreamSynchronize(g.stream);
        (void)hipGetLastError();
        h->poisoned = false;
    }
    const double *vs[3] = {vx, vy, vz};
    for (int ax = 0; ax < 3; ++ax) {
        int rc_ = upload(h, LJMD_R, ax, src[ax]);
        if (rc_ == LJMD_OK) rc_ = upload(h, LJMD_RU, ax, src[ax]);    // ru <- r (md_simulation_program.f90:229-231)
        if (rc_ == LJMD_OK) rc_ = upload(h, LJMD_V, ax, vs[ax]);
        if (rc_ != LJMD_OK) return rc_;
    }
    LJMD_HIP(h, hipMemsetAsync(plane(h, LJMD_A, 0), 0, 3 * h->total * sizeof(double), h->stream));
    LJMD_HIP(h, hipMemsetAsync(h->d_range, 0, h->B * sizeof(int32_t), h->stream));
    LJMD_HIP(h, hipStreamSynchronize(h->stream));
    h->have_state = true;
    h->have_accel = false;
    h->tcf_s = 0;                     // a new trajectory: no stored origin is live; the sums and counts stay
    return LJMD_OK;
}

int ljmd_batch_set_accel(ljmd_batch_t *h, const double *ax, const double *ay, const double *az)
{
    if (!h) return fail(nullptr, LJMD_ERR_INVALID_ARG, "ljmd_batch_set_accel: NULL handle");
    if (!h->have_state) return fail(h, LJMD_ERR_STATE, "ljmd_batch_set_accel: call ljmd_batch_set_state first");
    // NULL keeps a component, which is only valid accelerations once there are some: right after set_state every
    // component must be given
    if (!h->have_accel && !(ax && ay && az))
        return fail(h, LJMD_ERR_INVALID_ARG, "ljmd_batch_set_accel: no valid accelerations to keep; pass all three "
                                              "components (or call ljmd_batch_compute_forces)");
    LJMD_HIP(h, hipSetDevice(h->device));
    const double *src[3] = {ax, ay, az};
    for (int k = 0; k < 3; ++k)
        if (src[k]) {
            const int rc_ = upload(h, LJMD_A, k, src[k]);
            if (rc_ != LJMD_OK) return rc_;
        }
    LJMD_HIP(h, hipStreamSynchronize(h->stream));
    h->have_accel = true;
    return LJMD_OK;
}

int ljmd_batch_set_unwrapped(ljmd_batch_t *h, const double *ux, const double *uy, const double *uz)
{
    if (!h) return fail(nullptr, LJMD_ERR_INVALID_ARG, "ljmd_batch_set_unwrapped: NULL handle");
    if (!ux || !uy || !uz) return fail(h, LJMD_ERR_INVALID_ARG, "ljmd_batch_set_unwrapped: NULL array");
    if (!h->have_state) return fail(h, LJMD_ERR_STATE, "ljmd_batch_set_unwrapped: call ljmd_batch_set_state first");
    LJMD_HIP(h, hipSetDevice(h->device));
    const double *src[3] = {ux, uy, uz};
    for (int k = 0; k < 3; ++k) {
        const int rc_ = upload(h, LJMD_RU, k, src[k]);
        if (rc_ != LJMD_OK) return rc_;
    }
    LJMD_HIP(h, hipStreamSynchronize(h->stream));
    return LJMD_OK;
}

int ljmd_batch_get_state(ljmd_batch_t *h, double *rx, double *ry, double *rz, double *ux, double *uy, double *uz,
                         double *vx, double *vy, double *vz, double *ax, double *ay, double *az)
{
    if (!h) return fail(nullptr, LJMD_ERR_INVALID_ARG, "ljmd_batch_get_state: NULL handle");
    if (!h->have_state) return fail(h, LJMD_ERR_STATE, "ljmd_batch_get_state: no state has been set");
    LJMD_HIP(h, hipSetDevice(h->device));
    double *const dst[12] = {rx, ry, rz, ux, uy, uz, vx, vy, vz, ax, ay, az};
    for (int k = 0; k < 12; ++k)
        if (dst[k])
            LJMD_HIP(h, hipMemcpyAsync(dst[k], plane(h, k / 3, k % 3), h->total * sizeof(double),
                                        hipMemcpyDeviceToHost, h->stream));
    LJMD_HIP(h, hipStreamSynchronize(h->stream));
    return LJMD_OK;
}

int ljmd_batch_compute_forces(ljmd_batch_t *h, double *epot, double *d_epot, double *dd_epot)
{
    if (!h) return fail(nullptr, LJMD_ERR_INVALID_ARG, "ljmd_batch_compute_forces: NULL handle");
    if (!h->have_state) return fail(h, LJMD_ERR_STATE, "ljmd_batch_compute_forces: no state has been set");
    if (h->poisoned)
        return fail(h, LJMD_ERR_STATE, "ljmd_batch_compute_forces: handle poisoned by an earlier failure; call "
                                        "ljmd_batch_set_state");
    LJMD_HIP(h, hipSetDevice(h->device));
    int rc_ = run_groups(h, base_args(h, kModeForces), 0, 0, 0, nullptr, "ljmd_batch_compute_forces");
    if (rc_ != LJMD_OK) return rc_;
    rc_ = fetch_records(h, 1, "ljmd_batch_compute_forces");
    if (rc_ != LJMD_OK) return rc_;
    h->have_accel = true;
    for (size_t b = 0; b < h->B; ++b)
        combine(h, b, h->h_rec.data() + b * rec_words(h), epot ? epot + b : nullptr, nullptr,
                d_epot ? d_epot + b : nullptr, dd_epot ? dd_epot + b : nullptr);
    return LJMD_OK;
}

int ljmd_batch_kinetic_energy(ljmd_batch_t *h, double *ekin)
{
    if (!h || !ekin) return fail(h, LJMD_ERR_INVALID_ARG, "ljmd_batch_kinetic_energy: NULL argument");
    if (!h->have_state) return fail(h, LJMD_ERR_STATE, "ljmd_batch_kinetic_energy: no state has been set");
    if (h->poisoned)
        return fail(h, LJMD_ERR_STATE, "ljmd_batch_kinetic_energy: handle poisoned by an earlier failure; call "
                                        "ljmd_batch_set_state");
    LJMD_HIP(h, hipSetDevice(h->device));
    int rc_ = run_groups(h, base_args(h, kModeKinetic), 0, 0, 0, nullptr, "ljmd_batch_kinetic_energy");
    if (rc_ != LJMD_OK) return rc_;
    rc_ = fetch_records(h, 1, "ljmd_batch_kinetic_energy");
    if (rc_ != LJMD_OK) return rc_;
    for (size_t b = 0; b < h->B; ++b) {
        if (reproducible(h)) combine(h, b, h->h_rec.data() + b * kExactWords, nullptr, ekin + b, nullptr, nullptr);
        else ekin[b] = 0.5 * h->h_rec[b * kBatchRecWords + 2];   // md_simulation_program.f90:238-240
    }
    return LJMD_OK;
}

int ljmd_batch_steps(ljmd_batch_t *h, int32_t nsteps, int32_t sample_every, double *epot, double *ekin,
                     double *d_epot, double *dd_epot)
{
    if (!h) return fail(nullptr, LJMD_ERR_INVALID_ARG, "ljmd_batch_steps: NULL handle");
    if (nsteps < 0) return fail(h, LJMD_ERR_INVALID_ARG, "ljmd_batch_steps: nsteps < 0");
    const bool sampling = epot || ekin || d_epot || dd_epot;
    if (sampling) {
        if (sample_every < 1) return fail(h, LJMD_ERR_INVALID_ARG, "ljmd_batch_steps: sample_every must be >= 1");
        if (nsteps % sample_every != 0)
            return fail(h, LJMD_ERR_INVALID_ARG, "ljmd_batch_steps: nsteps %d is not a multiple of sample_every %d",
                         nsteps, sample_every);
        if (nsteps / sample_every > LJMD_MAX_PENDING_STEPS)
            return fail(h, LJMD_ERR_INVALID_ARG, "ljmd_batch_steps: %d samples exceed LJMD_MAX_PENDING_STEPS",
                         nsteps / sample_every);
    }
    if (!h->have_state) return fail(h, LJMD_ERR_STATE, "ljmd_batch_steps: no state has been set");
    if (!h->have_accel)
        return fail(h, LJMD_ERR_STATE, "ljmd_batch_steps: no valid accelerations; call ljmd_batch_compute_forces or "
                                        "ljmd_batch_set_accel first");
    if (h->poisoned)
        return fail(h, LJMD_ERR_STATE, "ljmd_batch_steps: handle poisoned by an earlier failure; call "
                                        "ljmd_batch_set_state");
    const int rdf_every = h->rdf_nbins > 0 ? h->rdf_every : 0;
    if (rdf_every > 0 && nsteps % rdf_every != 0)
        return fail(h, LJMD_ERR_INVALID_ARG, "ljmd_batch_steps: nsteps %d is not a multiple of the g(r) interval %d "
                                              "(ljmd_batch_rdf_configure: every)", nsteps, rdf_every);
    const int tcf_every = h->tcf_max_lag > 0 ? h->tcf_every : 0;
    if (tcf_every > 0 && nsteps % tcf_every != 0)
        return fail(h, LJMD_ERR_INVALID_ARG, "ljmd_batch_steps: nsteps %d is not a multiple of the MSD / VACF interval "
                                              "%d (ljmd_batch_tcf_configure: every)", nsteps, tcf_every);
    if (nsteps == 0) return LJMD_OK;
    LJMD_HIP(h, hipSetDevice(h->device));
    const size_t samples = sampling ? (size_t)(nsteps / sample_every) : 0;
    int rc_ = ensure_records(h, samples);
    if (rc_ != LJMD_OK) return rc_;
    BatchArgs a = base_args(h, kModeSteps);
    a.sample_every = sampling ? sample_every : 0;
    int32_t launches = 0;
    LJMD_HIP(h, hipEventRecord(h->ev[0], h->stream));
    rc_ = run_groups(h, a, nsteps, rdf_every, tcf_every, &launches, "ljmd_batch_steps");
    if (rc_ != LJMD_OK) return rc_;
    if (rdf_every > 0) h->rdf_snapshots += nsteps / rdf_every;
    if (tcf_every > 0)
        for (int k = 0; k < nsteps / tcf_every; ++k) tcf_advance(h);
    LJMD_HIP(h, hipEventRecord(h->ev[1], h->stream));
    rc_ = fetch_records(h, samples, "ljmd_batch_steps");
    if (rc_ != LJMD_OK) return rc_;
    float ms = 0.0f;
    LJMD_HIP(h, hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
    h->last_ms = ms;
    h->last_launches = launches;
    for (size_t s = 0; s < samples; ++s)
        for (size_t b = 0; b < h->B; ++b) {
            const size_t o = s * h->B + b;
            combine(h, b, h->h_rec.data() + o * rec_words(h), epot ? epot + o : nullptr, ekin ? ekin + o : nullptr,
                    d_epot ? d_epot + o : nullptr, dd_epot ? dd_epot + o : nullptr);
        }
    return LJMD_OK;
}

int ljmd_batch_set_precision(ljmd_batch_t *h, int32_t precision_mode)
{
    if (!h) return fail(nullptr, LJMD_ERR_INVALID_ARG, "ljmd_batch_set_precision: NULL handle");
    if (precision_mode != LJMD_PRECISION_FP64 && precision_mode != LJMD_PRECISION_FP64_REPRODUCIBLE)
        return fail(h, LJMD_ERR_INVALID_ARG, "ljmd_batch_set_precision: precision_mode %d not available for batches "
                                              "(LJMD_PRECISION_FP64 or LJMD_PRECISION_FP64_REPRODUCIBLE)", precision_mode);
    if (precision_mode == h->mode) return LJMD_OK;
    // the range words and a poisoned handle stay as they are: have_state = false below makes ljmd_batch_set_state the
    // only way on, and that call clears both
    h->mode = precision_mode;
    for (BatchGroup &g : h->groups) launch_shape(g.n_max, g.count, reproducible(h), &g.chunk, &g.steps_per_launch);
    h->have_state = false;            // the resident accelerations belong to the old mode
    h->have_accel = false;
    return LJMD_OK;
}

int ljmd_batch_set_tail_corrections(ljmd_batch_t *h, int32_t on)
{
    if (!h) return fail(nullptr, LJMD_ERR_INVALID_ARG, "ljmd_batch_set_tail_corrections: NULL handle");
    h->tail_on = on != 0;
    return LJMD_OK;
}

int ljmd_batch_profile_read(const ljmd_batch_t *h, double *kernel_ms, int32_t *launches)
{
    if (!h) return fail(nullptr, LJMD_ERR_INVALID_ARG, "ljmd_batch_profile_read: NULL handle");
    if (kernel_ms) *kernel_ms = h->last_ms;
    if (launches) *launches = h->last_launches;
    return LJMD_OK;
}

// ---- g(r) accumulation ---------------------------------------------------------------------------------------------

int ljmd_batch_rdf_configure(ljmd_batch_t *h, int32_t nbins, const double *rmax, int32_t every)
{
    static const char *who = "ljmd_batch_rdf_configure";
    if (!h) return fail(nullptr, LJMD_ERR_INVALID_ARG, "%s: NULL handle", who);
    if (nbins < 0 || nbins > kBatchRdfMaxBins)
        return fail(h, LJMD_ERR_INVALID_ARG, "%s: nbins = %d outside 1..%d (0 switches g(r) off)", who, nbins,
                     kBatchRdfMaxBins);
    if (every < 0) return fail(h, LJMD_ERR_INVALID_ARG, "%s: every must be >= 0", who);
    if (nbins > 0 && rmax)
        for (size_t b = 0; b < h->B; ++b)
            if (!(std::isfinite(rmax[b]) && rmax[b] > 0.0))
                return fail(h, LJMD_ERR_INVALID_ARG, "%s: replica %zu: rmax must be finite and > 0", who, b);
    LJMD_HIP(h, hipSetDevice(h->device));
    rdf_release(h);
    if (nbins == 0) return LJMD_OK;
    std::vector<BatchRdfReplica> table;
    try {
        table.resize(h->B);
    } catch (const std::bad_alloc &) {
        return fail(h, LJMD_ERR_ALLOC, "%s: out of host memory", who);
    }
    for (size_t b = 0; b < h->B; ++b) {
        BatchRdfReplica &e = table[b];
        e.rmax = rmax ? rmax[b] : 0.5 * h->rep[b].L;
        e.dr = e.rmax / nbins;                       // as the reference: dr = rmax / nbins
        e.inv_dr = 1.0 / e.dr;
    }
    const size_t hbytes = h->B * (size_t)nbins * sizeof(unsigned long long), tbytes = h->B * sizeof(BatchRdfReplica);
    auto body = [&]() -> int {
        if (hipMalloc(&h->d_rdf_hist, hbytes) != hipSuccess) {
            h->d_rdf_hist = nullptr;
            return fail(h, LJMD_ERR_ALLOC, "%s: cannot allocate %zu bytes of histograms", who, hbytes);
        }
        if (hipMalloc(&h->d_rdf_table, tbytes) != hipSuccess) {
            h->d_rdf_table = nullptr;
            return fail(h, LJMD_ERR_ALLOC, "%s: cannot allocate %zu bytes of the g(r) table", who, tbytes);
        }
        LJMD_HIP(h, hipMemsetAsync(h->d_rdf_hist, 0, hbytes, h->stream));
        LJMD_HIP(h, hipMemcpyAsync(h->d_rdf_table, table.data(), tbytes, hipMemcpyHostToDevice, h->stream));
        LJMD_HIP(h, hipStreamSynchronize(h->stream));    // table goes out of scope
        return LJMD_OK;
    };
    const int rc_ = body();
    if (rc_ != LJMD_OK) {
        rdf_release(h);
        return rc_;
    }
    h->rdf_nbins = nbins;
    h->rdf_every = every;
    return LJMD_OK;
}

int ljmd_batch_rdf_accumulate(ljmd_batch_t *h)
{
    static const char *who = "ljmd_batch_rdf_accumulate";
    if (!h) return fail(nullptr, LJMD_ERR_INVALID_ARG, "%s: NULL handle", who);
    if (h->rdf_nbins == 0) return fail(h, LJMD_ERR_STATE, "%s: call ljmd_batch_rdf_configure first", who);
    if (!h->have_state) return fail(h, LJMD_ERR_STATE, "%s: no state has been set", who);
    if (h->poisoned)
        return fail(h, LJMD_ERR_STATE, "%s: handle poisoned by an earlier failure; call ljmd_batch_set_state", who);
    LJMD_HIP(h, hipSetDevice(h->device));
    int32_t count = 0;
    for (const BatchGroup &g : h->groups) {
        const int rc_ = enqueue_rdf(h, g, h->stream, &count, who);
        if (rc_ != LJMD_OK) return rc_;
    }
    ++h->rdf_snapshots;
    return LJMD_OK;
}

int ljmd_batch_rdf_read(ljmd_batch_t *h, uint64_t *hist, int64_t *n_snapshots)
{
    static const char *who = "ljmd_batch_rdf_read";
    if (!h) return fail(nullptr, LJMD_ERR_INVALID_ARG, "%s: NULL handle", who);
    if (h->rdf_nbins == 0) return fail(h, LJMD_ERR_STATE, "%s: call ljmd_batch_rdf_configure first", who);
    static_assert(sizeof(uint64_t) == sizeof(unsigned long long), "histogram word");
    LJMD_HIP(h, hipSetDevice(h->device));
    if (hist)
        LJMD_HIP(h, hipMemcpyAsync(hist, h->d_rdf_hist, h->B * (size_t)h->rdf_nbins * sizeof(uint64_t),
                                    hipMemcpyDeviceToHost, h->stream));
    const hipError_t e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
        h->poisoned = true;
        return fail(h, LJMD_ERR_HIP, "%s: kernel or copy failed: %s; the handle is poisoned until ljmd_batch_set_state",
                     who, hipGetErrorString(e));
    }
    if (n_snapshots) *n_snapshots = h->rdf_snapshots;
    return LJMD_OK;
}

int ljmd_batch_rdf_reset(ljmd_batch_t *h)
{
    static const char *who = "ljmd_batch_rdf_reset";
    if (!h) return fail(nullptr, LJMD_ERR_INVALID_ARG, "%s: NULL handle", who);
    if (h->rdf_nbins == 0) return fail(h, LJMD_ERR_STATE, "%s: call ljmd_batch_rdf_configure first", who);
    LJMD_HIP(h, hipSetDevice(h->device));
    LJMD_HIP(h, hipMemsetAsync(h->d_rdf_hist, 0, h->B * (size_t)h->rdf_nbins * sizeof(unsigned long long), h->stream));
    h->rdf_snapshots = 0;
    return LJMD_OK;
}

// ---- MSD / VACF accumulation -----------------------------------------------------------------------------------------

int ljmd_batch_tcf_configure(ljmd_batch_t *h, int32_t max_lag, int32_t origin_stride, int32_t every)
{
    static const char *who = "ljmd_batch_tcf_configure";
    if (!h) return fail(nullptr, LJMD_ERR_INVALID_ARG, "%s: NULL handle", who);
    if (max_lag < 0 || max_lag > kBatchTcfMaxLag)
        return fail(h, LJMD_ERR_INVALID_ARG, "%s: max_lag = %d outside 1..%d (0 switches MSD / VACF off)", who, max_lag,
                     kBatchTcfMaxLag);
    if (every < 0) return fail(h, LJMD_ERR_INVALID_ARG, "%s: every must be >= 0", who);
    if (max_lag > 0 && origin_stride < 1) return fail(h, LJMD_ERR_INVALID_ARG, "%s: origin_stride must be >= 1", who);
    if (max_lag > 0 && max_lag / origin_stride + 1 > kBatchTcfMaxOrigins)
        return fail(h, LJMD_ERR_INVALID_ARG, "%s: max_lag / origin_stride + 1 = %d exceeds LJMD_BATCH_TCF_MAX_ORIGINS "
                                              "(%d)", who, max_lag / origin_stride + 1, kBatchTcfMaxOrigins);
    LJMD_HIP(h, hipSetDevice(h->device));
    tcf_release(h);
    if (max_lag == 0) return LJMD_OK;
    const int32_t slots = max_lag / origin_stride + 1;
    const size_t sbytes = h->B * 2 * ((size_t)max_lag + 1) * 3 * sizeof(uint64_t), fbytes = h->B * sizeof(int32_t);
    const size_t rbytes = (size_t)slots * 6 * h->total * sizeof(double);
    auto body = [&]() -> int {
        try {
            h->tcf_counts.assign((size_t)max_lag + 1, 0);
        } catch (const std::bad_alloc &) {
            return fail(h, LJMD_ERR_ALLOC, "%s: out of host memory", who);
        }
        if (hipMalloc(&h->d_tcf_sums, sbytes) != hipSuccess) {
            h->d_tcf_sums = nullptr;
            return fail(h, LJMD_ERR_ALLOC, "%s: cannot allocate %zu bytes of sums", who, sbytes);
        }
        if (hipMalloc(&h->d_tcf_range, fbytes) != hipSuccess) {
            h->d_tcf_range = nullptr;
            return fail(h, LJMD_ERR_ALLOC, "%s: cannot allocate %zu bytes of range words", who, fbytes);
        }
        if (hipMalloc(&h->d_tcf_ring, rbytes) != hipSuccess) {
            h->d_tcf_ring = nullptr;
            return fail(h, LJMD_ERR_ALLOC, "%s: cannot allocate %zu bytes of the origin ring (%d slots)", who, rbytes,
                         slots);
        }
        LJMD_HIP(h, hipMemsetAsync(h->d_tcf_sums, 0, sbytes, h->stream));
        LJMD_HIP(h, hipMemsetAsync(h->d_tcf_range, 0, fbytes, h->stream));
        LJMD_HIP(h, hipMemsetAsync(h->d_tcf_ring, 0, rbytes, h->stream));
        return LJMD_OK;
    };
    const int rc_ = body();
    if (rc_ != LJMD_OK) {
        (void)hipGetLastError();
        tcf_release(h);
        return rc_;
    }
    h->tcf_max_lag = max_lag;
    h->tcf_stride = origin_stride;
    h->tcf_every = every;
    h->tcf_slots = slots;
    return LJMD_OK;
}

int ljmd_batch_tcf_accumulate(ljmd_batch_t *h)
{
    static const char *who = "ljmd_batch_tcf_accumulate";
    if (!h) return fail(nullptr, LJMD_ERR_INVALID_ARG, "%s: NULL handle", who);
    if (h->tcf_max_lag == 0) return fail(h, LJMD_ERR_STATE, "%s: call ljmd_batch_tcf_configure first", who);
    if (!h->have_state) return fail(h, LJMD_ERR_STATE, "%s: no state has been set", who);
    if (h->poisoned)
        return fail(h, LJMD_ERR_STATE, "%s: handle poisoned by an earlier failure; call ljmd_batch_set_state", who);
    LJMD_HIP(h, hipSetDevice(h->device));
    int32_t count = 0;
    for (const BatchGroup &g : h->groups) {
        const int rc_ = enqueue_tcf(h, g, h->stream, h->tcf_s, &count, who);
        if (rc_ != LJMD_OK) return rc_;
    }
    tcf_advance(h);
    return LJMD_OK;
}

int ljmd_tcf_from_exact(const int64_t *words, int32_t n, int64_t count, double *out)
{
    if (!words || !out) return fail(nullptr, LJMD_ERR_INVALID_ARG, "ljmd_tcf_from_exact: NULL argument");
    if (n < 1 || count < 0) return fail(nullptr, LJMD_ERR_INVALID_ARG, "ljmd_tcf_from_exact: n must be >= 1, count >= 0");
    const uint64_t x[3] = {(uint64_t)words[0], (uint64_t)words[1], (uint64_t)words[2]};
    // one rounding of the integer, one division (n count < 2^53: the product is exact)
    *out = count == 0 ? 0.0 : ljmdk::fixed_to_double(x) / ((double)n * (double)count);
    return LJMD_OK;
}

int ljmd_batch_tcf_read(ljmd_batch_t *h, double *msd, double *vacf, int64_t *counts, int64_t *n_snapshots)
{
    static const char *who = "ljmd_batch_tcf_read";
    std::vector<uint64_t> w;
    const int rc_ = tcf_fetch(h, msd || vacf ? &w : nullptr, who);
    if (rc_ != LJMD_OK) return rc_;
    const size_t rows = (size_t)h->tcf_max_lag + 1;
    double *const dst[2] = {msd, vacf};
    for (size_t b = 0; b < h->B; ++b)
        for (int kind = 0; kind < 2; ++kind)
            for (size_t l = 0; dst[kind] && l < rows; ++l) {
                int64_t x[3];
                std::memcpy(x, w.data() + ((b * 2 + kind) * rows + l) * 3, sizeof x);
                (void)ljmd_tcf_from_exact(x, h->rep[b].n, h->tcf_counts[l], dst[kind] + b * rows + l);
            }
    if (counts) std::copy(h->tcf_counts.begin(), h->tcf_counts.end(), counts);
    if (n_snapshots) *n_snapshots = h->tcf_snapshots;
    return LJMD_OK;
}

int ljmd_batch_tcf_read_exact(ljmd_batch_t *h, int64_t *words, int64_t *counts, int64_t *n_snapshots)
{
    static const char *who = "ljmd_batch_tcf_read_exact";
    std::vector<uint64_t> w;
    const int rc_ = tcf_fetch(h, words ? &w : nullptr, who);
    if (rc_ != LJMD_OK) return rc_;
    if (words) std::memcpy(words, w.data(), w.size() * sizeof(uint64_t));
    if (counts) std::copy(h->tcf_counts.begin(), h->tcf_counts.end(), counts);
    if (n_snapshots) *n_snapshots = h->tcf_snapshots;
    return LJMD_OK;
}

int ljmd_batch_tcf_reset(ljmd_batch_t *h)
{
    static const char *who = "ljmd_batch_tcf_reset";
    if (!h) return fail(nullptr, LJMD_ERR_INVALID_ARG, "%s: NULL handle", who);
    if (h->tcf_max_lag == 0) return fail(h, LJMD_ERR_STATE, "%s: call ljmd_batch_tcf_configure first", who);
    LJMD_HIP(h, hipSetDevice(h->device));
    LJMD_HIP(h, hipMemsetAsync(h->d_tcf_sums, 0, tcf_sum_words(h) * sizeof(uint64_t), h->stream));
    LJMD_HIP(h, hipMemsetAsync(h->d_tcf_range, 0, h->B * sizeof(int32_t), h->stream));
    std::fill(h->tcf_counts.begin(), h->tcf_counts.end(), 0);
    h->tcf_s = 0;
    h->tcf_snapshots = 0;
    return LJMD_OK;
}

}  // extern "C"
