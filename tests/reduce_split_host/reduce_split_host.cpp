// reduce_split_host.cpp -- TEST INFRASTRUCTURE: what one engine step enqueues, and on which stream, with the pair kernel
// in two launches (LJMD_REDUCE_SPLIT, LaunchPlan::split_s1) and without.  Linked from the engine's host files, the fake HIP
// runtime (tests/fakehip) and this file's launchers, event records, stream waits and stream destructions, which write one
// line each into a transcript instead of reaching a device.  main builds an engine the way ljmd_create does, runs one
// step the way the step loop does (enqueue_drift, enqueue_forces) with the profile events on, releases the engine and
// compares the transcript with the sequence written out below.  No kernel runs.
#include "ljmd_engine.h"

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

namespace {

std::vector<std::string> g_log;
ljmd_t *g_h = nullptr;
int g_side_priority = 12345, g_least = 0;

std::string stream_name(hipStream_t s)
{
    if (g_h && s == g_h->stream) return "main";
    if (g_h && s == g_h->side_stream) return "side";
    return "other";
}

std::string event_name(hipEvent_t e)
{
    if (g_h && e == g_h->ev_side_go) return "side_go";
    if (g_h && e == g_h->ev_side_done) return "side_done";
    if (g_h)
        for (const EventSet &q : g_h->ev_pool)
            for (int k = 0; k < kEventsPerLaunch; ++k)
                if (q.e[k] == e) return "profile" + std::to_string(k);
    return "other";
}

hipError_t note(const std::string &what, hipStream_t s)
{
    g_log.push_back(what + " @" + stream_name(s));
    return hipSuccess;
}

}  // namespace

extern "C" {
hipError_t fakehip_hipEventRecord(hipEvent_t, hipStream_t);
hipError_t fakehip_hipStreamWaitEvent(hipStream_t, hipEvent_t, unsigned);
hipError_t fakehip_hipStreamDestroy(hipStream_t);

hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) { return note("record " + event_name(e), s); }
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned) { return note("wait " + event_name(e), s); }
hipError_t hipStreamDestroy(hipStream_t s)
{
    (void)note("destroy", s);
    return fakehip_hipStreamDestroy(s);
}
hipError_t hipDeviceGetStreamPriorityRange(int *least, int *greatest)
{
    *least = g_least = 1;            // numerically larger = lower priority
    *greatest = -2;
    return hipSuccess;
}
hipError_t hipStreamCreateWithPriority(hipStream_t *s, unsigned flags, int priority)
{
    g_side_priority = priority;
    return hipStreamCreateWithFlags(s, flags);
}
}  // extern "C"

namespace ljmdk {

hipError_t launch_pair_n3(const N3Args &a, dim3 grid, int, hipStream_t s)
{
    return note("pair_n3 by0=" + std::to_string(a.by0) + " slices=" + std::to_string(grid.y), s);
}
hipError_t launch_reduce_forces(const ReduceArgs &, bool, hipStream_t s) { return note("reduce_forces", s); }
hipError_t launch_reduce_forces_split(const ReduceArgs &a, int phase, hipStream_t s)
{
    return note("reduce_forces_split phase=" + std::to_string(phase) + " c_split=" + std::to_string(a.c_split) +
                " j_split=" + std::to_string(a.j_split), s);
}
hipError_t launch_drift_kick(const IntegrateArgs &, int, hipStream_t s) { return note("drift_kick", s); }
hipError_t launch_kick_finalize(const IntegrateArgs &, const FinalizeArgs &, bool, hipStream_t s) { return note("kick_finalize", s); }
hipError_t launch_kick(const IntegrateArgs &, bool, hipStream_t s) { return note("kick", s); }
hipError_t launch_finalize(const FinalizeArgs &, double *, hipStream_t s) { return note("finalize", s); }
hipError_t launch_tile_boxes(const GeometryArgs &, hipStream_t s) { return note("tile_boxes", s); }
hipError_t launch_tile_mask(const GeometryArgs &, hipStream_t s) { return note("tile_mask", s); }
hipError_t launch_tile_class(const GeometryArgs &, double, double, int, int, unsigned *, unsigned *, float *, hipStream_t s)
{
    return note("tile_class", s);
}
// not reached by a one-rank fp64 step of this size without a re-sort; present for the linker
hipError_t launch_pair_rows_generic(const PairArgs &, dim3, hipStream_t s) { return note("pair_rows_generic", s); }
hipError_t launch_pair_tiles(const PairArgs &, dim3, hipStream_t s) { return note("pair_tiles", s); }
hipError_t launch_pair_n3_f32(const N3Args &, dim3, hipStream_t s) { return note("pair_n3_f32", s); }
hipError_t launch_sum_blocks(const double *, double *, int, int, hipStream_t s) { return note("sum_blocks", s); }
hipError_t launch_tile_tail(const ReduceArgs &, const IntegrateArgs &, const FinalizeArgs &, const FinalizeArgs &, bool, bool,
                            hipStream_t s)
{
    return note("tile_tail", s);
}
hipError_t launch_pair_fixed(const FixedArgs &, dim3, hipStream_t s) { return note("pair_fixed", s); }
hipError_t launch_fixed_tail(const FixedTailArgs &, bool, bool, bool, hipStream_t s) { return note("fixed_tail", s); }
hipError_t launch_fixed_fold(const FixedFoldArgs &, hipStream_t s) { return note("fixed_fold", s); }
size_t kd_temp_bytes(int) { return 64; }
hipError_t launch_iota(int *, int, hipStream_t s) { return note("iota", s); }
hipError_t launch_iota_offset(int *, int, int, int, hipStream_t) { return hipSuccess; }     // allocate_engine
hipError_t kd_level(void *, size_t, const double *, double, unsigned long long *, unsigned long long *, int *, int *, int, int,
                    const int *, hipStream_t s)
{
    return note("kd_level", s);
}
hipError_t launch_gather3(const double *, double *, const int *, int, hipStream_t s) { return note("gather3", s); }
hipError_t launch_gather_perm(const int *, int *, const int *, int, hipStream_t s) { return note("gather_perm", s); }

}  // namespace ljmdk

namespace ljmdh { void release_resident(ljmd_t *) {} }

namespace {

int g_failed = 0;

void expect(const char *what, const std::vector<std::string> &want)
{
    bool same = g_log == want;
    std::printf("== %s: %s ==\n", what, same ? "ok" : "MISMATCH");
    for (size_t k = 0; k < std::max(g_log.size(), want.size()); ++k) {
        const std::string got = k < g_log.size() ? g_log[k] : "(nothing)", exp = k < want.size() ? want[k] : "(nothing)";
        std::printf("  %-62s %s\n", got.c_str(), got == exp ? "" : ("<- expected: " + exp).c_str());
    }
    if (!same) ++g_failed;
    g_log.clear();
}

void check(bool ok, const char *what)
{
    std::printf("%s: %s\n", what, ok ? "ok" : "FAILED");
    if (!ok) ++g_failed;
}

// ljmd_create without the device probe and the argument guards
ljmd_t *create(int n, double L, int mode)
{
    ljmd_t *h = new ljmd;
    h->n = n;
    h->mode = mode;
    static_cast<SimParams &>(*h) = derive_params(n, L, 0.005, 0.49 * L);
    h->knobs = read_knobs();
    if (plan_engine(*h, n, 1, mode, h->knobs, &h->plan) != LJMD_OK) std::abort();
    h->h_perm.resize(h->plan.P);
    for (int i = 0; i < h->plan.P; ++i) h->h_perm[i] = i;
    g_h = h;
    if (allocate_engine(h) != LJMD_OK) {
        std::printf("allocate_engine: %s\n", h->err.c_str());
        std::abort();
    }
    h->positions_compact = true;
    h->have_state = h->have_accel = true;
    h->profiling = true;
    g_log.clear();
    return h;
}

// one step as the step loop of ljmd_enqueue_steps issues it
void step(ljmd_t *h)
{
    EventSet *q = next_events(h);
    int rc = enqueue_drift(h, q);
    if (rc == LJMD_OK) rc = enqueue_forces(h, true, q, false);
    check(rc == LJMD_OK, "step enqueued");
}

size_t find(const std::vector<std::string> &log, const std::string &what)
{
    for (size_t k = 0; k < log.size(); ++k)
        if (log[k] == what) return k;
    return log.size();
}

}  // namespace

int main()
{
    const int n = 32768;             // 4-tile row groups, 130 slices of 2 units: a whole offset every 2 slices
    const double L = 34.5;
    setenv("LJMD_RESORT_EVERY", "1000", 1);

    // ---- path on: 16 of the 130 slices deferred -> s1 = 114, j1 = 114 * 2 / 4 = 57 ----
    setenv("LJMD_REDUCE_SPLIT", "16", 1);
    ljmd_t *h = create(n, L, LJMD_PRECISION_FP64);
    check(h->plan.nslab_n == 130 && h->plan.split_s1 == 114 && h->plan.split_j1 == 57, "plan: 130 slices, 114 + 16, 57 blocks");
    check(h->side_stream != nullptr && g_side_priority == g_least, "side stream created at the lowest priority");
    step(h);
    {
        const std::vector<std::string> log = g_log;
        const size_t go = find(log, "record side_go @main"), part2 = find(log, "pair_n3 by0=114 slices=16 @side");
        const size_t join = find(log, "wait side_done @main"), ph2 = find(log, "reduce_forces_split phase=2 c_split=114 j_split=57 @main");
        check(go < part2 && find(log, "wait side_go @side") < part2 && find(log, "tile_class @main") < go,
              "the second launch follows the event recorded behind the geometry pre-pass");
        check(join < ph2 && find(log, "record side_done @side") < join && part2 < find(log, "record side_done @side"),
              "phase 2 follows the join");
        check(join < find(log, "record profile3 @main") && find(log, "record profile3 @main") < ph2,
              "the pair interval ends behind the join, the reduce interval starts there");
    }
    expect("one step, path on", {
        "record profile0 @main",
        "drift_kick @main",
        "record profile1 @main",
        "tile_class @main",
        "record profile2 @main",
        "record side_go @main",
        "wait side_go @side",
        "pair_n3 by0=0 slices=114 @main",
        "pair_n3 by0=114 slices=16 @side",
        "reduce_forces_split phase=1 c_split=114 j_split=57 @main",
        "record side_done @side",
        "wait side_done @main",
        "record profile3 @main",
        "reduce_forces_split phase=2 c_split=114 j_split=57 @main",
        "kick_finalize @main",
        "record profile4 @main",
    });
    release(h);                      // (g_h still names the freed handle's streams: compared by address only)
    check(find(g_log, "destroy @side") < g_log.size() && find(g_log, "destroy @main") < g_log.size(),
          "the side stream is destroyed with the handle");
    {
        size_t side = 0;
        for (const std::string &l : g_log) side += l == "destroy @side";
        check(side == 1, "... once");
    }
    g_log.clear();
    g_h = nullptr;

    // ---- path off by the knob: today's sequence, no side stream ----
    setenv("LJMD_REDUCE_SPLIT", "0", 1);
    h = create(n, L, LJMD_PRECISION_FP64);
    check(h->plan.split_s1 == 0 && h->side_stream == nullptr && h->d_red_part == nullptr, "knob 0: no split, no side stream");
    step(h);
    const std::vector<std::string> off = {
        "record profile0 @main",
        "drift_kick @main",
        "record profile1 @main",
        "tile_class @main",
        "record profile2 @main",
        "pair_n3 by0=0 slices=130 @main",
        "record profile3 @main",
        "reduce_forces @main",
        "kick_finalize @main",
        "record profile4 @main",
    };
    expect("one step, path off", off);
    release(h);
    g_log.clear();
    g_h = nullptr;

    // ---- default at this size: off; the reproducible mode whatever the knob says: off ----
    unsetenv("LJMD_REDUCE_SPLIT");
    h = create(n, L, LJMD_PRECISION_FP64);
    check(h->plan.split_s1 == 0 && h->side_stream == nullptr, "default at n = 32768: off");
    step(h);
    expect("one step, default", off);
    release(h);
    g_log.clear();
    g_h = nullptr;
    setenv("LJMD_REDUCE_SPLIT", "16", 1);
    h = create(4096, 17.25, LJMD_PRECISION_FP64_REPRODUCIBLE);
    check(h->plan.split_s1 == 0 && h->side_stream == nullptr, "reproducible mode: off");
    release(h);
    h = create(4096, 17.25, LJMD_PRECISION_FP64);
    check(h->plan.split_s1 == 0 && h->side_stream == nullptr, "two-launch step of small systems: off");
    release(h);
    g_h = nullptr;

    std::printf(g_failed ? "FAILED: %d\n" : "all ok\n", g_failed);
    return g_failed ? 1 : 0;
}
