// batch_heatflux_host.cpp -- TEST INFRASTRUCTURE: the host code of the batch engine's heat flux
// (csrc/ljmd_heatflux_batch.cpp) and of the step loop that serves it, without a GPU.  Linked from the batch host files,
// ljmd_heatflux_batch.cpp, ljmd_stress_batch.cpp, ljmd_common.cpp, the fake HIP runtime (tests/fakehip) and its own
// definitions of the six launchers, which record what they are given instead of launching a kernel.  hipMalloc and
// hipFree of the fake runtime are wrapped at link time (-Wl,--wrap) so that the program counts the device allocations
// that are live.  The program checks itself -- the guard order, that a handle without configure launches what it launched
// before, the launch sequence with `every` on a two-group handle beside the pressure tensor (row, chunks, streams), the
// full-series refusal, what a failed launch leaves behind, and that reconfigure and destroy free everything -- prints one
// line per check that fails and "batch_heatflux_host: ok" when none did.  tests/test_batch_heatflux_host.py runs it under
// ASan and UBSan.
#include "ljmd.h"
#include "ljmd_batch_heatflux.h"
#include "ljmd_batch_host.h"
#include "ljmd_batch_stress.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

extern "C" {
hipError_t __real_hipMalloc(void **p, size_t n);
hipError_t __real_hipFree(void *p);
}

namespace {

int g_failures = 0;
long g_live = 0;                           // device allocations not yet freed
size_t g_fail_alloc_of = 0;                // != 0: a hipMalloc of exactly this many bytes fails

void check(bool ok, const char *what)
{
    if (ok) return;
    ++g_failures;
    std::printf("FAILED: %s\n", what);
}

// one recorded launch: kind 'B' steps / forces, 'F' the same in the reproducible mode, 'R' g(r), 'T' MSD / VACF,
// 'S' stress, 'H' heat flux
struct Launch {
    char kind;
    int g0, n_max, n_blocks;
    hipStream_t stream;
    int mode, step0, nsteps;               // 'B', 'F'
    long long row, rows;                   // 'S', 'H'
    bool operator==(const Launch &o) const
    {
        return kind == o.kind && g0 == o.g0 && n_max == o.n_max && n_blocks == o.n_blocks && stream == o.stream &&
               mode == o.mode && step0 == o.step0 && nsteps == o.nsteps && row == o.row && rows == o.rows;
    }
};
std::vector<Launch> g_log;
int g_fail_heatflux = 0;                   // k > 0: the k-th heat flux launch from now returns hipErrorLaunchFailure
int g_flag_heatflux = -1;                  // replica whose sticky word the next heat flux launch sets, as the kernel would

}  // namespace

extern "C" {

hipError_t __wrap_hipMalloc(void **p, size_t n)
{
    if (g_fail_alloc_of != 0 && n == g_fail_alloc_of) {
        *p = nullptr;
        return hipErrorOutOfMemory;
    }
    const hipError_t e = __real_hipMalloc(p, n);
    if (e == hipSuccess) ++g_live;
    return e;
}

hipError_t __wrap_hipFree(void *p)
{
    if (p) --g_live;
    return __real_hipFree(p);
}

}  // extern "C"

namespace ljmdb {

hipError_t launch_batch(const BatchArgs &a, int n_max, int n_blocks, hipStream_t s)
{
    g_log.push_back({'B', a.g0, n_max, n_blocks, s, a.mode, a.step0, a.nsteps, 0, 0});
    return hipSuccess;
}

hipError_t launch_batch_fixed(const BatchFixedArgs &a, int n_max, int n_blocks, hipStream_t s)
{
    g_log.push_back({'F', a.b.g0, n_max, n_blocks, s, a.b.mode, a.b.step0, a.b.nsteps, 0, 0});
    return hipSuccess;
}

hipError_t launch_batch_rdf(const BatchRdfArgs &a, int n_max, int n_blocks, hipStream_t s)
{
    g_log.push_back({'R', a.g0, n_max, n_blocks, s, 0, 0, 0, 0, 0});
    return hipSuccess;
}

hipError_t launch_batch_tcf(const BatchTcfArgs &a, int n_max, int n_blocks, hipStream_t s)
{
    g_log.push_back({'T', a.g0, n_max, n_blocks, s, 0, 0, 0, 0, 0});
    return hipSuccess;
}

hipError_t launch_batch_stress(const BatchStressArgs &a, int n_max, int n_blocks, hipStream_t s)
{
    g_log.push_back({'S', a.g0, n_max, n_blocks, s, 0, 0, 0, (long long)a.row, (long long)a.rows});
    return hipSuccess;
}

hipError_t launch_batch_heatflux(const BatchHeatfluxArgs &a, int n_max, int n_blocks, hipStream_t s)
{
    g_log.push_back({'H', a.g0, n_max, n_blocks, s, 0, 0, 0, (long long)a.row, (long long)a.rows});
    check(a.state && a.words && a.range && a.rep && a.B > 0 && a.plane > 0, "a heat flux launch has all its pointers");
    if (g_fail_heatflux > 0 && --g_fail_heatflux == 0) return hipErrorLaunchFailure;
    if (g_flag_heatflux >= 0) a.range[g_flag_heatflux] = 1;
    g_flag_heatflux = -1;
    // what the kernel would do, as far as the host can see it: something in every row it owns -- E_x, then P_y
    for (int k = 0; k < n_blocks; ++k) {
        const size_t b = (size_t)a.rep[a.g0 + k].b;
        uint64_t *const w = a.words + ((size_t)a.row * a.B + b) * kBatchHeatfluxWords;
        w[0] = 1000 + (uint64_t)b;
        w[3 * 4] = 7;
    }
    return hipSuccess;
}

}  // namespace ljmdb

namespace {

using ljmdb::kBatchHeatfluxWords;

bool message_has(const ljmd_batch_t *h, const char *text) { return std::strstr(ljmd_batch_last_error(h), text) != nullptr; }

int steps(ljmd_batch_t *h, int n) { return ljmd_batch_steps(h, n, 1, nullptr, nullptr, nullptr, nullptr); }

std::vector<Launch> only(char kind)
{
    std::vector<Launch> out;
    for (const Launch &l : g_log)
        if (l.kind == kind) out.push_back(l);
    return out;
}

int set_zero_state(ljmd_batch_t *h)
{
    const std::vector<double> zero(h->total, 0.0);
    const double *z = zero.data();
    return ljmd_batch_set_state(h, z, z, z, z, z, z);
}

int64_t count_of(ljmd_batch_t *h)
{
    int64_t n = -1;
    return ljmd_batch_heatflux_read_exact(h, nullptr, &n) == LJMD_OK ? n : -1;
}

// 1. the guards, in the order the header gives them
void guards()
{
    check(ljmd_batch_heatflux_configure(nullptr, -1, -1) == LJMD_ERR_INVALID_ARG, "configure: NULL handle first");
    check(std::strstr(ljmd_batch_last_error(nullptr), "ljmd_batch_heatflux_configure: NULL handle") != nullptr, "its message");
    check(ljmd_batch_heatflux_accumulate(nullptr) == LJMD_ERR_INVALID_ARG && ljmd_batch_heatflux_reset(nullptr) == LJMD_ERR_INVALID_ARG &&
              ljmd_batch_heatflux_read(nullptr, nullptr, nullptr, nullptr) == LJMD_ERR_INVALID_ARG &&
              ljmd_batch_heatflux_read_exact(nullptr, nullptr, nullptr) == LJMD_ERR_INVALID_ARG, "the other calls: NULL handle");
    ljmd_batch_t *h = nullptr;
    check(ljmd_batch_create(&h, 3, 108, 6.0, 0.005, 2.5, LJMD_PRECISION_FP64, 0) == LJMD_OK && h, "create");
    if (!h) return;
    const long base = g_live;
    check(ljmd_batch_heatflux_configure(h, -1, -1) == LJMD_ERR_INVALID_ARG && message_has(h, "max_snapshots = -1"),
          "max_snapshots < 0 before every");
    check(ljmd_batch_heatflux_configure(h, LJMD_BATCH_HEATFLUX_MAX_SNAPSHOTS + 1, 0) == LJMD_ERR_INVALID_ARG &&
              message_has(h, "max_snapshots"), "max_snapshots above the limit");
    check(ljmd_batch_heatflux_configure(h, 4, -1) == LJMD_ERR_INVALID_ARG && message_has(h, "every must be >= 0"), "every < 0");
    check(g_live == base && h->heatflux.max_snapshots == 0 && !h->heatflux.release, "the refused calls allocate nothing");
    check(ljmd_batch_heatflux_accumulate(h) == LJMD_ERR_STATE && message_has(h, "call ljmd_batch_heatflux_configure first"),
          "accumulate before configure");
    check(ljmd_batch_heatflux_read(h, nullptr, nullptr, nullptr) == LJMD_ERR_STATE &&
              ljmd_batch_heatflux_read_exact(h, nullptr, nullptr) == LJMD_ERR_STATE && ljmd_batch_heatflux_reset(h) == LJMD_ERR_STATE &&
              message_has(h, "call ljmd_batch_heatflux_configure first"), "read, read_exact, reset before configure");

    // the entry guard itself: g(r), MSD / VACF, the pressure tensor, the heat flux, a state, ..., each behind the last
    using namespace ljmdb;
    const unsigned all = kNeedRdf | kNeedTcf | kNeedStress | kNeedHeatflux | kNeedState | kNeedSound;
    check(enter(h, "who", all) == LJMD_ERR_STATE && message_has(h, "call ljmd_batch_rdf_configure first"), "g(r) is asked first");
    check(ljmd_batch_rdf_configure(h, 8, nullptr, 0) == LJMD_OK && enter(h, "who", all) == LJMD_ERR_STATE &&
              message_has(h, "call ljmd_batch_tcf_configure first"), "then MSD / VACF");
    check(ljmd_batch_tcf_configure(h, 4, 1, 0) == LJMD_OK && enter(h, "who", all) == LJMD_ERR_STATE &&
              message_has(h, "call ljmd_batch_stress_configure first"), "then the pressure tensor");
    check(ljmd_batch_stress_configure(h, 2, 0) == LJMD_OK && enter(h, "who", all) == LJMD_ERR_STATE &&
              message_has(h, "who: call ljmd_batch_heatflux_configure first"), "then the heat flux, behind the pressure tensor");
    const long others = g_live;
    check(ljmd_batch_heatflux_configure(h, 4, 2) == LJMD_OK && g_live == others + 2, "configure: the series and the range words");
    check(enter(h, "who", all) == LJMD_ERR_STATE && message_has(h, "no state has been set"), "then the state");
    check(ljmd_batch_heatflux_configure(h, -1, 0) == LJMD_ERR_INVALID_ARG && h->heatflux.max_snapshots == 4 && h->heatflux.every == 2 &&
              g_live == others + 2, "a failed guard keeps the earlier configuration");
    check(ljmd_batch_heatflux_accumulate(h) == LJMD_ERR_STATE && message_has(h, "no state has been set"), "accumulate before a state");
    check(set_zero_state(h) == LJMD_OK, "set_state");
    h->poisoned = true;
    check(ljmd_batch_heatflux_accumulate(h) == LJMD_ERR_STATE && message_has(h, "poisoned"), "accumulate on a poisoned handle");
    check(count_of(h) == 0, "a poisoned handle may still be read");
    h->poisoned = false;
    g_log.clear();
    check(ljmd_batch_heatflux_accumulate(h) == LJMD_OK && only('H').size() == 1 && g_log.size() == 1, "accumulate needs no accelerations");
    ljmd_batch_destroy(h);
    check(g_live == 0, "destroy frees everything");
}

// 2. without configure, with every == 0 and after configure(0) the step loop launches what it launched before
void off_is_off()
{
    const int32_t n[3] = {108, 1372, 108};
    const double L[3] = {6.0, 12.0, 6.0}, dt[3] = {0.005, 0.005, 0.005}, rc[3] = {2.5, 2.5, 2.5};
    ljmd_batch_t *h = nullptr;
    check(ljmd_batch_create_per_replica(&h, 3, n, L, dt, rc, LJMD_PRECISION_FP64, 0) == LJMD_OK && h, "create two groups");
    if (!h) return;
    check(set_zero_state(h) == LJMD_OK && ljmd_batch_compute_forces(h, nullptr, nullptr, nullptr) == LJMD_OK, "state");
    check(ljmd_batch_rdf_configure(h, 8, nullptr, 4) == LJMD_OK && ljmd_batch_tcf_configure(h, 4, 1, 6) == LJMD_OK &&
              ljmd_batch_stress_configure(h, 8, 3) == LJMD_OK, "g(r), MSD / VACF, the pressure tensor");
    auto restart = [&] {
        return ljmd_batch_tcf_reset(h) == LJMD_OK && ljmd_batch_stress_reset(h) == LJMD_OK && set_zero_state(h) == LJMD_OK &&
               ljmd_batch_compute_forces(h, nullptr, nullptr, nullptr) == LJMD_OK;
    };
    g_log.clear();
    check(steps(h, 12) == LJMD_OK, "steps without the heat flux");
    const std::vector<Launch> before = g_log;
    check(!before.empty() && only('H').empty() && !only('R').empty() && !only('T').empty() && only('S').size() == 8,
          "its transcript");
    check(ljmd_batch_heatflux_configure(h, 8, 0) == LJMD_OK, "configure with every == 0");
    check(restart(), "the same starting point");
    g_log.clear();
    check(steps(h, 12) == LJMD_OK && g_log == before, "every == 0: the same launches");
    check(ljmd_batch_heatflux_configure(h, 0, 0) == LJMD_OK && !h->heatflux.release && !h->heatflux.acc.enqueue, "configure(0) switches off");
    check(restart(), "the same starting point again");
    g_log.clear();
    check(steps(h, 12) == LJMD_OK && g_log == before, "switched off: the same launches");
    check(steps(h, 7) == LJMD_ERR_INVALID_ARG && message_has(h, "g(r) interval"), "the existing interval guard, unchanged");
    ljmd_batch_destroy(h);
    check(g_live == 0, "destroy frees everything (feature off)");
}

// 3. - 5. `every` on a two-group handle beside the pressure tensor; the full series; a failed launch
void sequence()
{
    const int32_t n[3] = {108, 1372, 108};
    const double L[3] = {6.0, 12.0, 6.0}, dt[3] = {0.005, 0.005, 0.005}, rc[3] = {2.5, 2.5, 2.5};
    ljmd_batch_t *h = nullptr;
    check(ljmd_batch_create_per_replica(&h, 3, n, L, dt, rc, LJMD_PRECISION_FP64, 0) == LJMD_OK && h, "create two groups");
    if (!h) return;
    check(h->groups.size() == 2 && h->concurrent, "two groups on streams of their own");
    check(set_zero_state(h) == LJMD_OK && ljmd_batch_compute_forces(h, nullptr, nullptr, nullptr) == LJMD_OK, "state");
    check(ljmd_batch_stress_configure(h, 64, 2) == LJMD_OK, "the pressure tensor beside it: configure(64, every = 2)");
    check(ljmd_batch_heatflux_configure(h, 6, 3) == LJMD_OK, "configure(6, every = 3)");

    g_log.clear();
    check(ljmd_batch_heatflux_accumulate(h) == LJMD_OK && count_of(h) == 1 && h->stress.count == 0, "accumulate");
    check(g_log.size() == 2 && g_log[0].kind == 'H' && g_log[1].kind == 'H' && g_log[0].row == 0 && g_log[1].row == 0 &&
              g_log[0].rows == 6 && g_log[0].stream == h->stream && g_log[1].stream == h->stream, "one launch per group, row 0, the handle's stream");
    check(g_log[0].g0 == 0 && g_log[0].n_blocks == 2 && g_log[0].n_max == 108 && g_log[1].g0 == 2 && g_log[1].n_blocks == 1 &&
              g_log[1].n_max == 1372, "each group's own table range and class");

    check(steps(h, 8) == LJMD_ERR_INVALID_ARG && message_has(h, "nsteps 8 is not a multiple of the heat flux interval 3 "
                                                                  "(ljmd_batch_heatflux_configure: every)"), "the interval guard names it");
    check(steps(h, 9) == LJMD_ERR_INVALID_ARG && message_has(h, "pressure tensor interval 2"), "the pressure tensor is asked before it");
    g_log.clear();
    check(steps(h, 6) == LJMD_OK && count_of(h) == 3 && h->stress.count == 3, "steps(6): two snapshots, three of the pressure tensor");
    int32_t launches = 0;
    check(ljmd_batch_profile_read(h, nullptr, &launches) == LJMD_OK && launches == (int32_t)g_log.size(), "profile_read counts them");
    for (const ljmdb::BatchGroup &g : h->groups) {
        std::vector<Launch> mine;
        for (const Launch &l : g_log)
            if (l.g0 >= (int)g.first && l.g0 < (int)(g.first + g.count)) mine.push_back(l);
        int k = 0, ks = 0;
        bool ok = !mine.empty();
        for (size_t i = 0; i < mine.size(); ++i) {
            ok = ok && mine[i].stream == g.stream && g.stream != h->stream;
            if (mine[i].kind == 'S') {
                ok = ok && mine[i].row == ks && mine[i].rows == 64;
                ++ks;
            }
            if (mine[i].kind != 'H') continue;
            // behind the step launch that ends at step (k + 1) * every -- at step 6 behind the pressure tensor's snapshot
            // of that step -- on the same stream; row = count + k
            size_t prev = i - 1;
            if (i > 0 && mine[prev].kind == 'S' && k == 1) --prev;
            ok = ok && i > 0 && mine[prev].kind == 'B' && mine[prev].step0 + mine[prev].nsteps == 3 * (k + 1) &&
                 mine[i].row == 1 + k && mine[i].rows == 6 && mine[i].n_blocks == (int)g.count && mine[i].n_max == g.n_max;
            ++k;
        }
        check(ok && k == 2 && ks == 3 && mine.back().kind == 'H',
              "a group's snapshots follow its steps 3 and 6 on its own stream, rows 1 and 2, the pressure tensor's its steps 2, 4, 6");
    }
    std::vector<int64_t> words((size_t)3 * 3 * kBatchHeatfluxWords);
    int64_t snaps = 0;
    check(ljmd_batch_heatflux_read_exact(h, words.data(), &snaps) == LJMD_OK && snaps == 3, "read_exact");
    for (int s = 0; s < 3; ++s)
        for (int b = 0; b < 3; ++b)
            check(words[((size_t)s * 3 + b) * kBatchHeatfluxWords] == 1000 + b, "sample-major rows, one per (snapshot, replica)");
    std::vector<double> j((size_t)3 * 3 * 3), parts((size_t)3 * 3 * 9);
    const double V0 = 6.0 * 6.0 * 6.0, V1 = 12.0 * 12.0 * 12.0;
    check(ljmd_batch_heatflux_read(h, j.data(), parts.data(), &snaps) == LJMD_OK && snaps == 3, "read");
    check(j[0] == 0.5 * (1000.0 * 0x1p-64) / V0 && j[1] == 7.0 * 0x1p-64 / V0 && j[2] == 0.0 &&
              j[3] == 0.5 * (1001.0 * 0x1p-64) / V1 && j[4] == 7.0 * 0x1p-64 / V1, "read: heatflux_doubles with the replica's own L");
    check(parts[0] == j[0] && parts[3 + 1] == j[1] && parts[9 + 0] == j[3] && parts[9 + 3 + 1] == j[4] && parts[6] == 0.0,
          "parts: convective, potential, collisional per replica");
    std::vector<double> j2(j.size(), -1.0);
    check(ljmd_batch_heatflux_read(h, j2.data(), nullptr, nullptr) == LJMD_OK && j2 == j, "read without parts");

    // the series is full for this call: refused before anything is launched, and nothing changes
    g_log.clear();
    check(steps(h, 12) == LJMD_ERR_STATE && message_has(h, "the heat flux series is full") && g_log.empty() && count_of(h) == 3 &&
              h->stress.count == 3 && !h->poisoned, "4 snapshots against room for 3: refused with zero launches");
    check(ljmd_batch_stress_configure(h, 0, 0) == LJMD_OK, "the pressure tensor off");
    check(steps(h, 9) == LJMD_OK && count_of(h) == 6 && only('H').size() == 6 && only('H').back().row == 5, "3 snapshots fit");
    g_log.clear();
    check(ljmd_batch_heatflux_accumulate(h) == LJMD_ERR_STATE && message_has(h, "series is full") && g_log.empty(), "accumulate on a full series");
    check(steps(h, 3) == LJMD_ERR_STATE && g_log.empty(), "steps on a full series");

    // the sticky range word: named, not poisoned, cleared by reset
    check(ljmd_batch_heatflux_reset(h) == LJMD_OK && count_of(h) == 0, "reset empties the series");
    g_flag_heatflux = 1;
    check(ljmd_batch_heatflux_accumulate(h) == LJMD_OK, "accumulate with a replica out of range");
    check(ljmd_batch_heatflux_read(h, nullptr, nullptr, nullptr) == LJMD_ERR_RANGE && message_has(h, "replica 1:") &&
              ljmd_batch_heatflux_read_exact(h, nullptr, nullptr) == LJMD_ERR_RANGE && !h->poisoned && steps(h, 3) == LJMD_OK,
          "LJMD_ERR_RANGE names the replica; the handle still steps");
    check(ljmd_batch_heatflux_reset(h) == LJMD_OK && count_of(h) == 0, "reset clears the word");

    // a failed heat flux launch half-way: poisoned, the count where it was
    check(steps(h, 3) == LJMD_OK && count_of(h) == 1, "one snapshot");
    g_fail_heatflux = 2;                             // the second snapshot of the first group
    g_log.clear();
    check(steps(h, 6) == LJMD_ERR_HIP && message_has(h, "heat flux launch failed") && message_has(h, "poisoned") && h->poisoned,
          "an injected launch failure poisons the handle");
    check(only('H').size() == 2, "(it failed at the second heat flux launch)");
    check(count_of(h) == 1 && h->heatflux.count == 1, "... and leaves the snapshot count alone");
    check(steps(h, 3) == LJMD_ERR_STATE && ljmd_batch_heatflux_accumulate(h) == LJMD_ERR_STATE, "poisoned until set_state");
    check(set_zero_state(h) == LJMD_OK && ljmd_batch_compute_forces(h, nullptr, nullptr, nullptr) == LJMD_OK && steps(h, 3) == LJMD_OK &&
              count_of(h) == 2, "set_state keeps configuration and series");

    // reconfigure and destroy free everything
    const long with = g_live;
    check(ljmd_batch_heatflux_configure(h, 100, 1) == LJMD_OK && g_live == with && count_of(h) == 0 && h->heatflux.every == 1,
          "reconfigure: the same number of allocations, an empty series");
    const size_t bytes = (size_t)216 * 3 * 7;
    g_fail_alloc_of = bytes;
    check(ljmd_batch_heatflux_configure(h, 7, 1) == LJMD_ERR_ALLOC && message_has(h, "cannot allocate 4536 bytes of the heat flux series") &&
              g_live == with - 2 && h->heatflux.max_snapshots == 0, "a failed allocation: LJMD_ERR_ALLOC with the feature off");
    g_fail_alloc_of = 0;
    check(ljmd_batch_heatflux_accumulate(h) == LJMD_ERR_STATE && steps(h, 5) == LJMD_OK, "off: stepping as before");
    check(ljmd_batch_heatflux_configure(h, 7, 1) == LJMD_OK && g_live == with, "configure again");
    check(ljmd_batch_heatflux_configure(h, 0, 0) == LJMD_OK && g_live == with - 2, "configure(0) frees it");
    check(ljmd_batch_heatflux_configure(h, 7, 1) == LJMD_OK && ljmd_batch_stress_configure(h, 7, 1) == LJMD_OK,
          "configure both once more: destroyed while configured");
    ljmd_batch_destroy(h);
    check(g_live == 0, "destroy frees everything (both features on)");
}

// chunks: more replicas of n = 4000 than the fp64 pair bound of one step allows in a launch
void chunks()
{
    const int32_t B = 1300;
    ljmd_batch_t *h = nullptr;
    check(ljmd_batch_create(&h, B, 4000, 20.0, 0.005, 2.5, LJMD_PRECISION_FP64, 0) == LJMD_OK && h, "create 1300 x 4000");
    if (!h) return;
    const size_t chunk = h->groups[0].rdf_chunk;
    check(h->groups.size() == 1 && chunk == 1250, "2e10 / 4000^2 = 1250 replicas per launch");
    check(set_zero_state(h) == LJMD_OK && ljmd_batch_heatflux_configure(h, 2, 0) == LJMD_OK, "state, configure");
    g_log.clear();
    check(ljmd_batch_heatflux_accumulate(h) == LJMD_OK && g_log.size() == 2 && g_log[0].g0 == 0 && g_log[0].n_blocks == 1250 &&
              g_log[1].g0 == 1250 && g_log[1].n_blocks == 50 && g_log[0].row == 0 && g_log[1].row == 0, "two chunks of one snapshot");
    ljmd_batch_destroy(h);
    check(g_live == 0, "destroy frees everything (many replicas)");
}

}  // namespace

int main()
{
    setenv("FAKEHIP_DEVICES", "1", 1);
    unsetenv("LJMD_BATCH_GROUP_STREAMS");
    guards();
    off_is_off();
    sequence();
    chunks();
    if (g_failures == 0) std::printf("batch_heatflux_host: ok\n");
    return g_failures == 0 ? 0 : 1;
}
