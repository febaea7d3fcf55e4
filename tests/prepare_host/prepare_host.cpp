// prepare_host.cpp -- TEST INFRASTRUCTURE: the host code of ljmd_batch_prepare (csrc/ljmd_prepare.cpp) without a GPU.
// Linked from the batch host files, ljmd_prepare.cpp, ljmd_common.cpp, the fake HIP runtime (tests/fakehip) and its own
// definitions of the six launchers, which record what they are given instead of launching a kernel; the force and
// kinetic-energy launchers write step records of known energies, so that the scale factors can be checked.  The program
// checks itself -- guards, the launches of one call, the scale factors, the warm-up without snapshots, what a target
// below the lattice energy and a failed launch leave behind -- prints one line per check that fails and "prepare_host:
// ok" when none did.  tests/test_batch_prepare_host.py runs it under ASan and UBSan.
#include "ljmd.h"
#include "ljmd_batch_prepare.h"

#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {

int g_failures = 0;
int g_init = 0, g_scale = 0, g_batch_steps = 0, g_batch_forces = 0, g_batch_kinetic = 0, g_rdf = 0, g_tcf = 0;
int g_fail_init = 0;                       // 1: the next init launch returns hipErrorLaunchFailure
std::vector<int> g_init_seen;              // how often each replica was covered by an init launch
std::vector<int32_t> g_seeds;              // seeds[b] as the init launcher saw them
std::vector<double> g_scales;              // scale[b] as the scale launcher saw them
std::vector<double> g_twice_ekin;          // what the kinetic-energy launcher reports per replica: sum v^2

void check(bool ok, const char *what)
{
    if (ok) return;
    ++g_failures;
    std::printf("FAILED: %s\n", what);
}

}  // namespace

namespace ljmdb {

hipError_t launch_batch(const BatchArgs &a, int, int n_blocks, hipStream_t)
{
    if (a.mode == kModeSteps) ++g_batch_steps;
    for (int k = 0; k < n_blocks && a.mode != kModeSteps; ++k) {
        const BatchReplica &rp = a.rep[a.g0 + k];
        double *rec = a.rec + (size_t)rp.b * kBatchRecWords;
        for (int w = 0; w < kBatchRecWords; ++w) rec[w] = 0.0;       // epot = 0 with the tail corrections off
        if (a.mode == kModeKinetic) rec[2] = g_twice_ekin[(size_t)rp.b];
    }
    if (a.mode == kModeForces) ++g_batch_forces;
    if (a.mode == kModeKinetic) ++g_batch_kinetic;
    return hipSuccess;
}

hipError_t launch_batch_fixed(const BatchFixedArgs &, int, int, hipStream_t) { return hipErrorInvalidValue; }

hipError_t launch_batch_rdf(const BatchRdfArgs &, int, int, hipStream_t)
{
    ++g_rdf;
    return hipSuccess;
}

hipError_t launch_batch_tcf(const BatchTcfArgs &, int, int, hipStream_t)
{
    ++g_tcf;
    return hipSuccess;
}

hipError_t launch_batch_init(const BatchInitArgs &a, int n_max, int n_blocks, hipStream_t)
{
    ++g_init;
    if (g_fail_init > 0 && --g_fail_init == 0) return hipErrorLaunchFailure;
    for (int k = 0; k < n_blocks; ++k) {
        const BatchReplica &rp = a.rep[a.g0 + k];
        check(rp.n <= n_max && batch_class(rp.n) == batch_class(n_max), "an init launch holds one kernel class");
        ++g_init_seen[(size_t)rp.b];
        g_seeds[(size_t)rp.b] = a.seeds[rp.b];
    }
    return hipSuccess;
}

hipError_t launch_batch_scale(const BatchScaleArgs &a, int, int n_blocks, hipStream_t)
{
    ++g_scale;
    for (int k = 0; k < n_blocks; ++k) {
        const BatchReplica &rp = a.rep[a.g0 + k];
        g_scales[(size_t)rp.b] = a.scale[rp.b];
    }
    return hipSuccess;
}

}  // namespace ljmdb

namespace {

bool message_has(const ljmd_batch_t *h, const char *text) { return std::strstr(ljmd_batch_last_error(h), text) != nullptr; }

int steps1(ljmd_batch_t *h) { return ljmd_batch_steps(h, 1, 1, nullptr, nullptr, nullptr, nullptr); }

}  // namespace

int main()
{
    setenv("FAKEHIP_DEVICES", "1", 1);
    const int32_t B = 5;
    const int32_t n[B] = {32, 108, 500, 2048, 2916};                 // four kernel classes, 108 and 500 in one
    const double L[B] = {4.0, 5.0, 9.0, 14.0, 16.0}, dt[B] = {0.005, 0.005, 0.005, 0.005, 0.005};
    const double rc[B] = {1.9, 2.4, 4.0, 6.0, 7.0};
    g_init_seen.assign(B, 0);
    g_seeds.assign(B, 0);
    g_scales.assign(B, 0.0);
    g_twice_ekin = {2.0, 4.0, 6.0, 8.0, 10.0};                       // ekin0 = 1 .. 5
    ljmd_batch_t *h = nullptr;
    check(ljmd_batch_create_per_replica(&h, B, n, L, dt, rc, LJMD_PRECISION_FP64, 0) == LJMD_OK && h, "create");
    if (!h) return 1;
    check(ljmd_batch_set_tail_corrections(h, 0) == LJMD_OK, "tail corrections off");
    const int32_t seeds[B] = {7, -8, 9, INT32_MAX, 1618033};
    const double target[B] = {4.0, 8.0, 12.0, 16.0, 20.0};           // target - 0 = 4 ekin0: scale 2
    double epot0[B], ekin0[B];

    // argument guards: the handle is left as it was (here: without a state)
    check(ljmd_batch_prepare(nullptr, seeds, target, 0, nullptr, nullptr) == LJMD_ERR_INVALID_ARG, "NULL handle");
    check(ljmd_batch_prepare(h, nullptr, target, 0, nullptr, nullptr) == LJMD_ERR_INVALID_ARG, "NULL seeds");
    check(ljmd_batch_prepare(h, seeds, nullptr, 0, nullptr, nullptr) == LJMD_ERR_INVALID_ARG, "NULL targets");
    check(ljmd_batch_prepare(h, seeds, target, -1, nullptr, nullptr) == LJMD_ERR_INVALID_ARG && message_has(h, "warmup_steps"),
          "warmup_steps < 0");
    int32_t bad_seeds[B] = {7, -8, INT32_MIN, 1, 2};
    check(ljmd_batch_prepare(h, bad_seeds, target, 0, nullptr, nullptr) == LJMD_ERR_INVALID_ARG && message_has(h, "replica 2:"),
          "seed INT32_MIN names its replica");
    check(g_init == 0 && steps1(h) == LJMD_ERR_STATE, "the guards launch nothing and set no state");

    // one call: every replica initialised once, with its own seed; one force and one kinetic pass; scale 2
    check(ljmd_batch_prepare(h, seeds, target, 0, epot0, ekin0) == LJMD_OK, "prepare");
    check(g_init == 4 && g_scale == 4 && g_batch_forces == 4 && g_batch_kinetic == 4 && g_batch_steps == 0,
          "one launch per kernel class of each kind");
    for (int b = 0; b < B; ++b) {
        check(g_init_seen[(size_t)b] == 1 && g_seeds[(size_t)b] == seeds[b], "each replica once, with its own seed");
        check(epot0[b] == 0.0 && ekin0[b] == b + 1.0 && g_scales[(size_t)b] == 2.0, "energies and scale factor");
    }
    check(steps1(h) == LJMD_OK, "state and accelerations are valid afterwards");

    // the warm-up takes no snapshot, whatever the accumulators' intervals; they are back afterwards
    check(ljmd_batch_rdf_configure(h, 16, nullptr, 1) == LJMD_OK && ljmd_batch_tcf_configure(h, 4, 1, 1) == LJMD_OK, "configure");
    g_batch_steps = g_rdf = g_tcf = 0;
    check(ljmd_batch_prepare(h, seeds, target, 3, nullptr, nullptr) == LJMD_OK, "prepare with a warm-up");
    check(g_batch_steps >= 4 && g_rdf == 0 && g_tcf == 0, "warm-up steps without snapshots");
    int64_t rdf_snaps = -1, tcf_snaps = -1;
    std::vector<uint64_t> hist((size_t)B * 16);
    check(ljmd_batch_rdf_read(h, hist.data(), &rdf_snaps) == LJMD_OK && rdf_snaps == 0, "no g(r) snapshot counted");
    check(ljmd_batch_tcf_read(h, nullptr, nullptr, nullptr, &tcf_snaps) == LJMD_OK && tcf_snaps == 0, "no MSD / VACF snapshot counted");
    check(ljmd_batch_steps(h, 2, 1, nullptr, nullptr, nullptr, nullptr) == LJMD_OK && g_rdf > 0, "the intervals are back");
    check(ljmd_batch_rdf_read(h, hist.data(), &rdf_snaps) == LJMD_OK && rdf_snaps == 2, "two g(r) snapshots");
    check(ljmd_batch_tcf_read(h, nullptr, nullptr, nullptr, &tcf_snaps) == LJMD_OK && tcf_snaps == 2, "two MSD / VACF snapshots");

    // a target at or below the lattice energy, and nothing to rescale: the first such replica, no state, no poison
    double low[B] = {4.0, 0.0, 12.0, -1.0, 20.0};
    check(ljmd_batch_prepare(h, seeds, low, 0, nullptr, nullptr) == LJMD_ERR_INVALID_ARG && message_has(h, "replica 1:"),
          "target - epot0 <= 0 names the first replica");
    check(steps1(h) == LJMD_ERR_STATE && message_has(h, "no state"), "the handle has no state then");
    g_twice_ekin[2] = 0.0;
    check(ljmd_batch_prepare(h, seeds, target, 0, nullptr, nullptr) == LJMD_ERR_INVALID_ARG && message_has(h, "replica 2:") &&
              message_has(h, "ekin0"), "ekin0 <= 0 names the replica");
    g_twice_ekin[2] = 6.0;
    check(ljmd_batch_prepare(h, seeds, target, 0, nullptr, nullptr) == LJMD_OK && steps1(h) == LJMD_OK, "usable again");

    // a failed launch poisons the handle; the next prepare clears the poison
    g_fail_init = 2;
    check(ljmd_batch_prepare(h, seeds, target, 0, nullptr, nullptr) == LJMD_ERR_HIP && message_has(h, "poisoned"), "failed launch");
    check(steps1(h) == LJMD_ERR_STATE, "poisoned");
    check(ljmd_batch_prepare(h, seeds, target, 0, nullptr, nullptr) == LJMD_OK && steps1(h) == LJMD_OK, "recovered");

    // a replica that is no FCC lattice
    ljmd_batch_destroy(h);
    const int32_t n2[2] = {500, 100};
    check(ljmd_batch_create_per_replica(&h, 2, n2, L, dt, rc, LJMD_PRECISION_FP64, 0) == LJMD_OK && h, "create 500 + 100");
    if (!h) return 1;
    check(ljmd_batch_prepare(h, seeds, target, 0, nullptr, nullptr) == LJMD_ERR_INVALID_ARG && message_has(h, "replica 1:") &&
              message_has(h, "n = 100"), "n = 100 is not 4 k^3");
    ljmd_batch_destroy(h);
    if (g_failures == 0) std::printf("prepare_host: ok\n");
    return g_failures == 0 ? 0 : 1;
}
