// ljmd_batch.cpp -- host side of the batch engine (include/ljmd.h: ljmd_batch_*): B independent replicas on one
// device, each with its own (n, L, dt, rc) (ljmd_batch_create: all the same), stepped by one kernel (ljmd_batch.hip)
// with one workgroup per replica.  Handle lifecycle, guards, device state, launch planning per kernel class, the step
// loop and the combination of the per-replica step records, in the fp64 mode and in the reproducible mode (exact integer
// records, a sticky range flag per replica: ljmd_batch_fixed.hip).  The accumulators the step loop serves are
// ljmd_batch_rdf.cpp (g(r)), ljmd_batch_tcf.cpp (MSD / VACF) and, through the handle alone, ljmd_stress_batch.cpp (the
// pressure tensor), ljmd_heatflux_batch.cpp (the heat flux), ljmd_vanhove_batch.cpp (the van Hove function) and
// ljmd_rhok_batch.cpp (the density modes);
// ljmd_batch_host.h is what these files share.
#include "ljmd_batch_host.h"

using namespace ljmdb;

int ljmdb::enter(ljmd_batch *h, const char *who, unsigned need)
{
    if (!h) return fail(nullptr, LJMD_ERR_INVALID_ARG, "%s: NULL handle", who);
    auto state = [&](const char *what) { return fail(h, LJMD_ERR_STATE, "%s: %s", who, what); };
    if ((need & kNeedRdf) && h->rdf.nbins == 0) return state("call ljmd_batch_rdf_configure first");
    if ((need & kNeedTcf) && h->tcf.max_lag == 0) return state("call ljmd_batch_tcf_configure first");
    if ((need & kNeedStress) && h->stress.max_snapshots == 0) return state("call ljmd_batch_stress_configure first");
    if ((need & kNeedHeatflux) && h->heatflux.max_snapshots == 0) return state("call ljmd_batch_heatflux_configure first");
    if ((need & kNeedVanhove) && h->vanhove.max_lag == 0) return state("call ljmd_batch_vanhove_configure first");
    if ((need & kNeedRhok) && h->rhok.max_snapshots == 0) return state("call ljmd_batch_rhok_configure first");
    if ((need & kNeedState) && !h->have_state) return state("no state has been set");
    if ((need & kNeedAccel) && !h->have_accel)
        return state("no valid accelerations; call ljmd_batch_compute_forces or ljmd_batch_set_accel first");
    if ((need & kNeedSound) && h->poisoned) return state("handle poisoned by an earlier failure; call ljmd_batch_set_state");
    if (need & kNeedDevice) LJMD_HIP(h, hipSetDevice(h->device));
    return LJMD_OK;
}

int ljmdb::accumulate_now(ljmd_batch *h, const BatchAccumulator &a, const char *who)
{
    int32_t count = 0;
    for (const BatchGroup &g : h->groups) LJMD_TRY(a.enqueue(h, g, h->stream, 0, &count, who));
    a.ran(h, 1);
    return LJMD_OK;
}

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

size_t rec_words(const ljmd_batch *h) { return reproducible(h) ? kExactWords : kBatchRecWords; }

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
    LJMD_TRY(device_alloc(h, &h->d_rec, words * sizeof(double), "ljmd_batch", "step records"));
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
    if (s != hipSuccess)
        return poison(h, LJMD_ERR_HIP, "ljmd_batch: kernel or copy failed: %s; the handle is poisoned until "
                                       "ljmd_batch_set_state", hipGetErrorString(s));
    if (reproducible(h))
        for (size_t b = 0; b < h->B; ++b)
            if (h->h_range[b] != 0)     // poisons, unlike the MSD / VACF range word (tcf_fetch): the trajectory is spoilt
                return poison(h, LJMD_ERR_RANGE, "%s: reproducible mode: replica %zu: a pair or velocity term was not "
                                                 "finite or |term| >= 2^40 (particles closer than about 0.12 sigma?); "
                                                 "the handle is poisoned until ljmd_batch_set_state", who, b);
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

// one pass of the kernel over every replica in `mode`: nsteps steps (kModeSteps) or one evaluation.  Group by group,
// launches of at most chunk replicas and steps_per_launch steps, in the order steps-outer, replicas-inner.  With
// concurrent groups every group runs on its own stream between a fork from and a join into the handle's stream, so
// what the handle's stream does next (the record copy) follows all of them.  A failed launch poisons the handle.
// An accumulator with every > 0 (kModeSteps only): a launch ends at the steps every, 2 every, ..., and the group's
// enqueue follows it on the same stream (the caller does the host's share afterwards: BatchAccumulator::ran); with
// every == 0 throughout, the launch sequence is the one without accumulators.
int run_groups(ljmd_batch *h, BatchArgs a, int nsteps, const BatchAccumulators &acc, int32_t *launches, const char *who)
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
            for (const BatchAccumulator &x : acc)
                if (x.every > 0) len = std::min(len, x.every - s0 % x.every);
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
                if (e == hipSuccess) continue;
                if (steps)
                    return poison(h, LJMD_ERR_HIP, "%s: launch at step %d failed: %s; the handle is poisoned until "
                                                   "ljmd_batch_set_state", who, s0, hipGetErrorString(e));
                // the forces / kinetic form of the message does not say so, yet the handle is poisoned
                return poison(h, LJMD_ERR_HIP, "%s: launch failed: %s", who, hipGetErrorString(e));
            }
            for (const BatchAccumulator &x : acc)
                if (x.every > 0 && (s0 + len) % x.every == 0)
                    LJMD_TRY(x.enqueue(h, g, s, (s0 + len) / x.every - 1, &count, who));
        }
        if (h->concurrent) {
            LJMD_HIP(h, hipEventRecord(g.done, s));
            LJMD_HIP(h, hipStreamWaitEvent(h->stream, g.done, 0));
        }
    }
    if (launches) *launches = count;
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
        LJMD_TRY(host_alloc(h, who, [&] {
            h->rep = std::move(reps);
            h->offsets.resize(h->B + 1);
            table.reserve(h->B);
        }));
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
        const size_t tbytes = h->B * sizeof(BatchReplica), fbytes = h->B * sizeof(int32_t);
        LJMD_TRY(device_alloc(h, &h->d_state, 12 * h->total * sizeof(double), who, "replica state"));
        LJMD_TRY(device_alloc(h, &h->d_table, tbytes, who, "the replica table"));
        if (hipMemcpyAsync(h->d_table, table.data(), tbytes, hipMemcpyHostToDevice, h->stream) != hipSuccess ||
            hipStreamSynchronize(h->stream) != hipSuccess)
            return fail(h, LJMD_ERR_HIP, "%s: cannot upload the replica table", who);
        LJMD_TRY(host_alloc(h, who, [&] { h->h_range.assign(h->B, 0); }));
        LJMD_TRY(device_alloc(h, &h->d_range, fbytes, who, "range flags"));
        if (hipMemsetAsync(h->d_range, 0, fbytes, h->stream) != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess)
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
    LJMD_TRY(ljmdh::probe_device(device, "ljmd_batch_create"));
    std::vector<BatchRep> reps;
    LJMD_TRY(host_alloc(nullptr, "ljmd_batch_create",
                        [&] { reps.assign((size_t)n_replicas, derive(n, box_length, dt, rc)); }));
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
    LJMD_TRY(ljmdh::probe_device(device, who));
    std::vector<BatchRep> reps;
    LJMD_TRY(host_alloc(nullptr, who, [&] {
        reps.reserve((size_t)n_replicas);
        for (int32_t b = 0; b < n_replicas; ++b) reps.push_back(derive(n[b], box_length[b], dt[b], rc[b]));
    }));
    return create_handle(out, std::move(reps), device, who);
}

int ljmd_batch_offsets(const ljmd_batch_t *h, int64_t *offsets)
{
    if (!h || !offsets) return fail(h, LJMD_ERR_INVALID_ARG, "ljmd_batch_offsets: NULL argument");
    std::copy(h->offsets.begin(), h->offsets.end(), offsets);
    return LJMD_OK;
}

// (the order is kept as it grew: the state once the handle's stream is idle, the rest once the groups' streams are)
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
    if (h->stress.release) h->stress.release(h);
    if (h->heatflux.release) h->heatflux.release(h);
    if (h->vanhove.release) h->vanhove.release(h);
    if (h->rhok.release) h->rhok.release(h);
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
    LJMD_TRY(enter(h, "ljmd_batch_set_state", 0));
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
        LJMD_TRY(upload(h, LJMD_R, ax, src[ax]));
        LJMD_TRY(upload(h, LJMD_RU, ax, src[ax]));    // ru <- r (md_simulation_program.f90:229-231)
        LJMD_TRY(upload(h, LJMD_V, ax, vs[ax]));
    }
    LJMD_HIP(h, hipMemsetAsync(plane(h, LJMD_A, 0), 0, 3 * h->total * sizeof(double), h->stream));
    LJMD_HIP(h, hipMemsetAsync(h->d_range, 0, h->B * sizeof(int32_t), h->stream));
    LJMD_HIP(h, hipStreamSynchronize(h->stream));
    h->have_state = true;
    h->have_accel = false;
    h->tcf.s = 0;                     // a new trajectory: no stored origin is live; the sums and counts stay
    h->vanhove.s = 0;
    return LJMD_OK;
}

int ljmd_batch_set_accel(ljmd_batch_t *h, const double *ax, const double *ay, const double *az)
{
    LJMD_TRY(enter(h, "ljmd_batch_set_accel", 0));
    if (!h->have_state) return fail(h, LJMD_ERR_STATE, "ljmd_batch_set_accel: call ljmd_batch_set_state first");
    // NULL keeps a component, which is only valid accelerations once there are some: right after set_state every
    // component must be given
    if (!h->have_accel && !(ax && ay && az))
        return fail(h, LJMD_ERR_INVALID_ARG, "ljmd_batch_set_accel: no valid accelerations to keep; pass all three "
                                              "components (or call ljmd_batch_compute_forces)");
    LJMD_HIP(h, hipSetDevice(h->device));
    const double *src[3] = {ax, ay, az};
    for (int k = 0; k < 3; ++k)
        if (src[k]) LJMD_TRY(upload(h, LJMD_A, k, src[k]));
    LJMD_HIP(h, hipStreamSynchronize(h->stream));
    h->have_accel = true;
    return LJMD_OK;
}

int ljmd_batch_set_unwrapped(ljmd_batch_t *h, const double *ux, const double *uy, const double *uz)
{
    LJMD_TRY(enter(h, "ljmd_batch_set_unwrapped", 0));
    if (!ux || !uy || !uz) return fail(h, LJMD_ERR_INVALID_ARG, "ljmd_batch_set_unwrapped: NULL array");
    if (!h->have_state) return fail(h, LJMD_ERR_STATE, "ljmd_batch_set_unwrapped: call ljmd_batch_set_state first");
    LJMD_HIP(h, hipSetDevice(h->device));
    const double *src[3] = {ux, uy, uz};
    for (int k = 0; k < 3; ++k) LJMD_TRY(upload(h, LJMD_RU, k, src[k]));
    LJMD_HIP(h, hipStreamSynchronize(h->stream));
    return LJMD_OK;
}

int ljmd_batch_get_state(ljmd_batch_t *h, double *rx, double *ry, double *rz, double *ux, double *uy, double *uz,
                         double *vx, double *vy, double *vz, double *ax, double *ay, double *az)
{
    LJMD_TRY(enter(h, "ljmd_batch_get_state", kNeedState | kNeedDevice));
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
    static const char *who = "ljmd_batch_compute_forces";
    LJMD_TRY(enter(h, who, kNeedState | kNeedSound | kNeedDevice));
    LJMD_TRY(run_groups(h, base_args(h, kModeForces), 0, {}, nullptr, who));
    LJMD_TRY(fetch_records(h, 1, who));
    h->have_accel = true;
    for (size_t b = 0; b < h->B; ++b)
        combine(h, b, h->h_rec.data() + b * rec_words(h), epot ? epot + b : nullptr, nullptr,
                d_epot ? d_epot + b : nullptr, dd_epot ? dd_epot + b : nullptr);
    return LJMD_OK;
}

int ljmd_batch_kinetic_energy(ljmd_batch_t *h, double *ekin)
{
    static const char *who = "ljmd_batch_kinetic_energy";
    if (!h || !ekin) return fail(h, LJMD_ERR_INVALID_ARG, "%s: NULL argument", who);
    LJMD_TRY(enter(h, who, kNeedState | kNeedSound | kNeedDevice));
    LJMD_TRY(run_groups(h, base_args(h, kModeKinetic), 0, {}, nullptr, who));
    LJMD_TRY(fetch_records(h, 1, who));
    for (size_t b = 0; b < h->B; ++b) {
        if (reproducible(h)) combine(h, b, h->h_rec.data() + b * kExactWords, nullptr, ekin + b, nullptr, nullptr);
        else ekin[b] = 0.5 * h->h_rec[b * kBatchRecWords + 2];   // md_simulation_program.f90:238-240
    }
    return LJMD_OK;
}

int ljmd_batch_steps(ljmd_batch_t *h, int32_t nsteps, int32_t sample_every, double *epot, double *ekin,
                     double *d_epot, double *dd_epot)
{
    static const char *who = "ljmd_batch_steps";
    LJMD_TRY(enter(h, who, 0));       // the argument guards come before the state guards, the device after all of them
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
    LJMD_TRY(enter(h, who, kNeedState | kNeedAccel | kNeedSound));
    const BatchAccumulators acc = accumulators(h);
    for (const BatchAccumulator &x : acc)
        if (x.every > 0 && nsteps % x.every != 0)
            return fail(h, LJMD_ERR_INVALID_ARG, "%s: nsteps %d is not a multiple of the %s interval %d "
                                                  "(ljmd_batch_%s_configure: every)", who, nsteps, x.name, x.every, x.tag);
    for (const BatchAccumulator &x : acc)
        if (x.every > 0 && x.room) LJMD_TRY(x.room(h, nsteps / x.every, who));
    if (nsteps == 0) return LJMD_OK;
    LJMD_HIP(h, hipSetDevice(h->device));
    const size_t samples = sampling ? (size_t)(nsteps / sample_every) : 0;
    LJMD_TRY(ensure_records(h, samples));
    BatchArgs a = base_args(h, kModeSteps);
    a.sample_every = sampling ? sample_every : 0;
    int32_t launches = 0;
    LJMD_HIP(h, hipEventRecord(h->ev[0], h->stream));
    LJMD_TRY(run_groups(h, a, nsteps, acc, &launches, who));
    for (const BatchAccumulator &x : acc)
        if (x.every > 0) x.ran(h, nsteps / x.every);
    LJMD_HIP(h, hipEventRecord(h->ev[1], h->stream));
    LJMD_TRY(fetch_records(h, samples, who));
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
    LJMD_TRY(enter(h, "ljmd_batch_set_precision", 0));
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
    LJMD_TRY(enter(h, "ljmd_batch_set_tail_corrections", 0));
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

}  // extern "C"
