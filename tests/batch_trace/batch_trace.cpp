// batch_trace.cpp -- TEST INFRASTRUCTURE: a transcript of what the batch engine's host code does, without a GPU.  The
// program is linked from the batch host files, ljmd_common.cpp, the fake HIP runtime (tests/fakehip) and its own
// definitions of the four launchers of ljmd_batch.h, which print their arguments instead of launching a kernel.  main
// walks the C ABI of include/ljmd.h (ljmd_batch_*): every guard in the order the code checks it, the launch sequence of
// both precision modes with and without the two accumulators, and what follows a failed launch.  Each call's return code
// and message are printed; tests/test_batch_trace.py compares the output byte for byte with expected.txt, under ASan and
// UBSan.  No kernel runs: device-derived numbers mean nothing here and are not printed.
#include "ljmd.h"
#include "ljmd_batch.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace {

enum Launcher { kBatch, kFixed, kRdf, kTcf, kLaunchers };
int g_fail_in[kLaunchers] = {0, 0, 0, 0};   // k > 0: the launcher's k-th call from now returns hipErrorLaunchFailure
int g_flag_fixed = -1, g_flag_tcf = -1;     // replica whose sticky range word the launcher's next call sets, as a kernel would
std::vector<hipStream_t> g_streams;         // in order of first appearance since the handle was created

int stream_no(hipStream_t s)
{
    for (size_t k = 0; k < g_streams.size(); ++k)
        if (g_streams[k] == s) return (int)k;
    g_streams.push_back(s);
    return (int)g_streams.size() - 1;
}

hipError_t launched(Launcher which)
{
    std::printf("\n");
    return g_fail_in[which] > 0 && --g_fail_in[which] == 0 ? hipErrorLaunchFailure : hipSuccess;
}

void print_batch(const char *name, const ljmdb::BatchArgs &a, int n_max, int n_blocks, hipStream_t s)
{
    std::printf("  %s stream=%d g0=%d n_max=%d n_blocks=%d mode=%d nsteps=%d step0=%d sample_every=%d", name, stream_no(s),
                a.g0, n_max, n_blocks, a.mode, a.nsteps, a.step0, a.sample_every);
}

}  // namespace

namespace ljmdb {

hipError_t launch_batch(const BatchArgs &a, int n_max, int n_blocks, hipStream_t s)
{
    print_batch("launch_batch", a, n_max, n_blocks, s);
    return launched(kBatch);
}

hipError_t launch_batch_fixed(const BatchFixedArgs &a, int n_max, int n_blocks, hipStream_t s)
{
    print_batch("launch_batch_fixed", a.b, n_max, n_blocks, s);
    std::printf(" rec=%d range=%d", a.rec != nullptr, a.range != nullptr);
    if (g_flag_fixed >= 0 && a.range) a.range[g_flag_fixed] = 1;
    g_flag_fixed = -1;
    return launched(kFixed);
}

hipError_t launch_batch_rdf(const BatchRdfArgs &a, int n_max, int n_blocks, hipStream_t s)
{
    std::printf("  launch_batch_rdf stream=%d g0=%d n_max=%d n_blocks=%d nbins=%d", stream_no(s), a.g0, n_max, n_blocks,
                a.nbins);
    return launched(kRdf);
}

hipError_t launch_batch_tcf(const BatchTcfArgs &a, int n_max, int n_blocks, hipStream_t s)
{
    std::printf("  launch_batch_tcf stream=%d g0=%d n_max=%d n_blocks=%d max_lag=%d stride=%d slots=%d n_live=%d "
                "lag_first=%d slot_first=%d store_slot=%d", stream_no(s), a.g0, n_max, n_blocks, a.max_lag, a.stride,
                a.slots, a.n_live, a.lag_first, a.slot_first, a.store_slot);
    if (g_flag_tcf >= 0 && a.range) a.range[g_flag_tcf] = 1;
    g_flag_tcf = -1;
    return launched(kTcf);
}

}  // namespace ljmdb

namespace {

// the return code of one C ABI call and, when it failed, the message; a trailing " (file:line)" of LJMD_HIP is cut
int report(const char *call, int rc, const ljmd_batch_t *h)
{
    std::printf("%s -> %d\n", call, rc);
    if (rc != 0) {
        std::string msg = ljmd_batch_last_error(h);
        const size_t open = msg.rfind(" (");
        if (!msg.empty() && msg.back() == ')' && open != std::string::npos && msg.find(".cpp:", open) != std::string::npos)
            msg.erase(open);
        std::printf("  error: %s\n", msg.c_str());
    }
    return rc;
}
#define CALL(h, expr) report(#expr, (expr), (h))

void section(const char *name) { std::printf("== %s ==\n", name); }

void print_i64(const char *name, const std::vector<int64_t> &v)
{
    std::printf("  %s =", name);
    for (int64_t x : v) std::printf(" %lld", (long long)x);
    std::printf("\n");
}

// a handle with the buffers its calls need: zero positions and velocities pass every guard of ljmd_batch_set_state
struct Batch {
    ljmd_batch_t *h = nullptr;
    int B = 0;
    std::vector<int64_t> off;
    std::vector<double> zero, out[4];
    const double *z() const { return zero.data(); }

    void adopt(int n_replicas)
    {
        g_streams.clear();
        B = n_replicas;
        off.assign((size_t)B + 1, 0);
        CALL(h, ljmd_batch_offsets(h, off.data()));
        if (B <= 8) print_i64("offsets", off);
        else std::printf("  offsets[%d] = %lld\n", B, (long long)off[(size_t)B]);
        zero.assign((size_t)off[(size_t)B], 0.0);
    }
    int set_state() { return CALL(h, ljmd_batch_set_state(h, z(), z(), z(), z(), z(), z())); }
    // ljmd_batch_steps with all four scalars sampled (sample_every > 0) or none, then the launches it counted
    void steps(int nsteps, int sample_every)
    {
        std::printf("steps(%d, sample_every %d)\n", nsteps, sample_every);
        int rc;
        if (sample_every > 0) {
            for (auto &o : out) o.assign((size_t)(nsteps / sample_every) * B, 0.0);
            rc = CALL(h, ljmd_batch_steps(h, nsteps, sample_every, out[0].data(), out[1].data(), out[2].data(), out[3].data()));
        } else {
            rc = CALL(h, ljmd_batch_steps(h, nsteps, 0, nullptr, nullptr, nullptr, nullptr));
        }
        int32_t launches = -1;
        if (rc == 0 && ljmd_batch_profile_read(h, nullptr, &launches) == 0) std::printf("  launches = %d\n", launches);
    }
    int forces()
    {
        for (auto &o : out) o.assign((size_t)B, 0.0);
        return CALL(h, ljmd_batch_compute_forces(h, out[0].data(), out[2].data(), out[3].data()));
    }
    int kinetic()
    {
        out[1].assign((size_t)B, 0.0);
        return CALL(h, ljmd_batch_kinetic_energy(h, out[1].data()));
    }
    void rdf_read(int nbins)
    {
        std::vector<uint64_t> hist((size_t)B * nbins);
        int64_t snaps = -1;
        if (CALL(h, ljmd_batch_rdf_read(h, hist.data(), &snaps)) == 0) std::printf("  n_snapshots = %lld\n", (long long)snaps);
    }
    void tcf_read(int max_lag)
    {
        const size_t rows = (size_t)max_lag + 1;
        std::vector<double> msd((size_t)B * rows), vacf((size_t)B * rows);
        std::vector<int64_t> counts(rows, -1), words((size_t)B * 2 * rows * 3);
        int64_t snaps = -1;
        if (CALL(h, ljmd_batch_tcf_read(h, msd.data(), vacf.data(), counts.data(), &snaps)) == 0) {
            print_i64("counts", counts);
            std::printf("  n_snapshots = %lld\n", (long long)snaps);
        }
        counts.assign(rows, -1);
        if (CALL(h, ljmd_batch_tcf_read_exact(h, words.data(), counts.data(), &snaps)) == 0) {
            print_i64("counts", counts);
            std::printf("  n_snapshots = %lld\n", (long long)snaps);
        }
    }
    void destroy()
    {
        ljmd_batch_destroy(h);
        h = nullptr;
    }
};

// kernel classes 0 0 1 2 3 3 4 in replica order 0 4 0 1 2 3 3
const int32_t kHetN[] = {32, 4000, 108, 500, 1000, 1372, 2048};
const int kHetB = sizeof kHetN / sizeof kHetN[0];

// the first B of them
void create_heterogeneous(Batch *t, int B)
{
    std::vector<double> L((size_t)B), dt((size_t)B, 0.005), rc((size_t)B, 2.5);
    for (int b = 0; b < B; ++b) L[(size_t)b] = 8.0 + b;
    CALL(nullptr, ljmd_batch_create_per_replica(&t->h, B, kHetN, L.data(), dt.data(), rc.data(), LJMD_PRECISION_FP64, 0));
    t->adopt(B);
}

void guards_without_handle()
{
    section("guards: creation and NULL handles");
    ljmd_batch_t *h = nullptr;
    CALL(nullptr, ljmd_batch_create(nullptr, 2, 8, 10.0, 0.005, 2.5, LJMD_PRECISION_FP64, 0));
    CALL(nullptr, ljmd_batch_create(&h, 2, 0, 10.0, 0.005, 2.5, LJMD_PRECISION_FP64, 0));
    CALL(nullptr, ljmd_batch_create(&h, 2, 8, 0.0, 0.005, 2.5, LJMD_PRECISION_FP64, 0));
    CALL(nullptr, ljmd_batch_create(&h, 2, 8, 10.0, 0.005, 0.0, LJMD_PRECISION_FP64, 0));
    CALL(nullptr, ljmd_batch_create(&h, 2, 8, 10.0, 0.005, 5.0, LJMD_PRECISION_FP64, 0));
    CALL(nullptr, ljmd_batch_create(&h, 2, 8, 10.0, 0.0, 2.5, LJMD_PRECISION_FP64, 0));
    CALL(nullptr, ljmd_batch_create(&h, 0, 8, 10.0, 0.005, 2.5, LJMD_PRECISION_FP64, 0));
    CALL(nullptr, ljmd_batch_create(&h, 2, LJMD_BATCH_MAX_N + 1, 10.0, 0.005, 2.5, LJMD_PRECISION_FP64, 0));
    CALL(nullptr, ljmd_batch_create(&h, 2, 8, 10.0, 0.005, 2.5, LJMD_PRECISION_FP64_REPRODUCIBLE, 0));
    CALL(nullptr, ljmd_batch_create(&h, 2, 8, 10.0, 0.005, 5.0 * (1.0 - 1e-12), LJMD_PRECISION_FP64, 0));
    CALL(nullptr, ljmd_batch_create(&h, 2, 8, 10.0, 0.005, 2.5, LJMD_PRECISION_FP64, 1));
    CALL(nullptr, ljmd_batch_create(&h, 2, 8, 10.0, 0.005, 2.5, LJMD_PRECISION_FP64, -1));

    int32_t n[2] = {8, 16};
    double L[2] = {10.0, 12.0}, dt[2] = {0.005, 0.004}, rc[2] = {2.5, 3.0};
    CALL(nullptr, ljmd_batch_create_per_replica(nullptr, 2, n, L, dt, rc, LJMD_PRECISION_FP64, 0));
    CALL(nullptr, ljmd_batch_create_per_replica(&h, 0, n, L, dt, rc, LJMD_PRECISION_FP64, 0));
    CALL(nullptr, ljmd_batch_create_per_replica(&h, 2, nullptr, L, dt, rc, LJMD_PRECISION_FP64, 0));
    CALL(nullptr, ljmd_batch_create_per_replica(&h, 2, n, L, dt, nullptr, LJMD_PRECISION_FP64, 0));
    CALL(nullptr, ljmd_batch_create_per_replica(&h, 2, n, L, dt, rc, LJMD_PRECISION_FP64_REPRODUCIBLE, 0));
    n[1] = 0;
    CALL(nullptr, ljmd_batch_create_per_replica(&h, 2, n, L, dt, rc, LJMD_PRECISION_FP64, 0));
    n[1] = LJMD_BATCH_MAX_N + 1;
    CALL(nullptr, ljmd_batch_create_per_replica(&h, 2, n, L, dt, rc, LJMD_PRECISION_FP64, 0));
    n[1] = 16;
    L[1] = -1.0;
    CALL(nullptr, ljmd_batch_create_per_replica(&h, 2, n, L, dt, rc, LJMD_PRECISION_FP64, 0));
    L[1] = 12.0;
    dt[0] = 0.0;
    CALL(nullptr, ljmd_batch_create_per_replica(&h, 2, n, L, dt, rc, LJMD_PRECISION_FP64, 0));
    dt[0] = 0.005;
    rc[1] = NAN;
    CALL(nullptr, ljmd_batch_create_per_replica(&h, 2, n, L, dt, rc, LJMD_PRECISION_FP64, 0));
    rc[1] = 6.0;
    CALL(nullptr, ljmd_batch_create_per_replica(&h, 2, n, L, dt, rc, LJMD_PRECISION_FP64, 0));
    rc[1] = 3.0;
    CALL(nullptr, ljmd_batch_create_per_replica(&h, 2, n, L, dt, rc, LJMD_PRECISION_FP64, 3));
    {   // 2^31 particles in all
        const int32_t many = 1 << 19;
        std::vector<int32_t> nn((size_t)many, LJMD_BATCH_MAX_N);
        std::vector<double> LL((size_t)many, 10.0), dd((size_t)many, 0.005), rr((size_t)many, 2.5);
        CALL(nullptr, ljmd_batch_create_per_replica(&h, many, nn.data(), LL.data(), dd.data(), rr.data(), LJMD_PRECISION_FP64, 0));
    }
    std::printf("handle after the failed creations: %s\n", h ? "set" : "NULL");

    double x = 0.0;
    int64_t i64 = 0;
    int32_t i32 = 0;
    uint64_t u64 = 0;
    ljmd_batch_destroy(nullptr);
    CALL(nullptr, ljmd_batch_offsets(nullptr, &i64));
    CALL(nullptr, ljmd_batch_set_state(nullptr, &x, &x, &x, &x, &x, &x));
    CALL(nullptr, ljmd_batch_set_accel(nullptr, &x, &x, &x));
    CALL(nullptr, ljmd_batch_set_unwrapped(nullptr, &x, &x, &x));
    CALL(nullptr, ljmd_batch_get_state(nullptr, &x, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0));
    CALL(nullptr, ljmd_batch_compute_forces(nullptr, &x, &x, &x));
    CALL(nullptr, ljmd_batch_kinetic_energy(nullptr, &x));
    CALL(nullptr, ljmd_batch_steps(nullptr, 1, 1, &x, &x, &x, &x));
    CALL(nullptr, ljmd_batch_set_precision(nullptr, LJMD_PRECISION_FP64));
    CALL(nullptr, ljmd_batch_set_tail_corrections(nullptr, 1));
    CALL(nullptr, ljmd_batch_profile_read(nullptr, &x, &i32));
    CALL(nullptr, ljmd_batch_rdf_configure(nullptr, 8, nullptr, 0));
    CALL(nullptr, ljmd_batch_rdf_accumulate(nullptr));
    CALL(nullptr, ljmd_batch_rdf_read(nullptr, &u64, &i64));
    CALL(nullptr, ljmd_batch_rdf_reset(nullptr));
    CALL(nullptr, ljmd_batch_tcf_configure(nullptr, 4, 1, 0));
    CALL(nullptr, ljmd_batch_tcf_accumulate(nullptr));
    CALL(nullptr, ljmd_batch_tcf_read(nullptr, &x, &x, &i64, &i64));
    CALL(nullptr, ljmd_batch_tcf_read_exact(nullptr, &i64, &i64, &i64));
    CALL(nullptr, ljmd_batch_tcf_reset(nullptr));
    int64_t w[3] = {0, 1, 0};
    CALL(nullptr, ljmd_tcf_from_exact(nullptr, 1, 1, &x));
    CALL(nullptr, ljmd_tcf_from_exact(w, 0, 1, &x));
    CALL(nullptr, ljmd_tcf_from_exact(w, 1, -1, &x));
    CALL(nullptr, ljmd_tcf_from_exact(w, 4, 0, &x));
    std::printf("  out = %g\n", x);
    CALL(nullptr, ljmd_tcf_from_exact(w, 4, 2, &x));   // 2^0 / (4 * 2): host arithmetic
    std::printf("  out = %g\n", x);
}

// every guard of a live handle, in the order the code checks them; a uniform handle of 3 replicas of 8 particles
void guards_with_handle()
{
    section("guards: a live handle, in call order");
    Batch t;
    CALL(nullptr, ljmd_batch_create(&t.h, 3, 8, 10.0, 0.005, 2.5, LJMD_PRECISION_FP64, 0));
    t.adopt(3);
    ljmd_batch_t *h = t.h;
    const double *z = t.z();
    double x[24] = {};
    CALL(h, ljmd_batch_offsets(h, nullptr));
    // before any state
    CALL(h, ljmd_batch_set_accel(h, z, z, z));
    CALL(h, ljmd_batch_set_unwrapped(h, z, z, nullptr));
    CALL(h, ljmd_batch_set_unwrapped(h, z, z, z));
    CALL(h, ljmd_batch_get_state(h, x, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0));
    CALL(h, ljmd_batch_compute_forces(h, x, x, x));
    CALL(h, ljmd_batch_kinetic_energy(h, nullptr));
    CALL(h, ljmd_batch_kinetic_energy(h, x));
    CALL(h, ljmd_batch_steps(h, -1, 1, x, x, x, x));
    CALL(h, ljmd_batch_steps(h, 4, 0, x, nullptr, nullptr, nullptr));
    CALL(h, ljmd_batch_steps(h, 5, 2, nullptr, x, nullptr, nullptr));
    CALL(h, ljmd_batch_steps(h, LJMD_MAX_PENDING_STEPS + 1, 1, nullptr, nullptr, x, nullptr));
    CALL(h, ljmd_batch_steps(h, 4, 2, nullptr, nullptr, nullptr, x));
    CALL(h, ljmd_batch_steps(h, 0, 0, nullptr, nullptr, nullptr, nullptr));
    CALL(h, ljmd_batch_rdf_accumulate(h));
    CALL(h, ljmd_batch_rdf_read(h, nullptr, nullptr));
    CALL(h, ljmd_batch_rdf_reset(h));
    CALL(h, ljmd_batch_tcf_accumulate(h));
    CALL(h, ljmd_batch_tcf_read(h, nullptr, nullptr, nullptr, nullptr));
    CALL(h, ljmd_batch_tcf_read_exact(h, nullptr, nullptr, nullptr));
    CALL(h, ljmd_batch_tcf_reset(h));
    // configuration ranges
    double rmax[3] = {4.0, 0.0, 4.0};
    CALL(h, ljmd_batch_rdf_configure(h, -1, nullptr, 0));
    CALL(h, ljmd_batch_rdf_configure(h, 8193, nullptr, 0));
    CALL(h, ljmd_batch_rdf_configure(h, 8, nullptr, -1));
    CALL(h, ljmd_batch_rdf_configure(h, 8, rmax, 0));
    rmax[1] = INFINITY;
    CALL(h, ljmd_batch_rdf_configure(h, 8, rmax, 0));
    CALL(h, ljmd_batch_rdf_configure(h, 0, rmax, 0));   // off: rmax is not looked at
    rmax[1] = 3.0;
    CALL(h, ljmd_batch_rdf_configure(h, 8, rmax, 3));
    CALL(h, ljmd_batch_tcf_configure(h, -1, 1, 0));
    CALL(h, ljmd_batch_tcf_configure(h, LJMD_BATCH_TCF_MAX_LAG + 1, 1, 0));
    CALL(h, ljmd_batch_tcf_configure(h, 4, 1, -1));
    CALL(h, ljmd_batch_tcf_configure(h, 4, 0, 0));
    CALL(h, ljmd_batch_tcf_configure(h, LJMD_BATCH_TCF_MAX_ORIGINS, 1, 0));
    CALL(h, ljmd_batch_tcf_configure(h, 0, 0, 0));      // off: the stride is not looked at
    CALL(h, ljmd_batch_tcf_configure(h, LJMD_BATCH_TCF_MAX_ORIGINS - 1, 1, 0));
    CALL(h, ljmd_batch_tcf_configure(h, 4, 2, 2));
    // configured, still no state
    CALL(h, ljmd_batch_rdf_accumulate(h));
    CALL(h, ljmd_batch_tcf_accumulate(h));
    CALL(h, ljmd_batch_steps(h, 6, 0, nullptr, nullptr, nullptr, nullptr));
    // set_state's own guards
    std::vector<double> bad(t.zero);
    CALL(h, ljmd_batch_set_state(h, z, z, z, z, z, nullptr));
    bad[8 + 3] = NAN;
    CALL(h, ljmd_batch_set_state(h, z, bad.data(), z, z, z, z));
    bad[8 + 3] = 24.0;
    CALL(h, ljmd_batch_set_state(h, z, z, bad.data(), z, z, z));
    t.set_state();
    // state, no accelerations
    CALL(h, ljmd_batch_set_accel(h, z, nullptr, z));
    CALL(h, ljmd_batch_steps(h, 6, 0, nullptr, nullptr, nullptr, nullptr));
    CALL(h, ljmd_batch_set_accel(h, z, z, z));
    CALL(h, ljmd_batch_set_accel(h, nullptr, z, nullptr));
    // interval multiples: g(r) every 3, MSD / VACF every 2
    CALL(h, ljmd_batch_steps(h, 4, 0, nullptr, nullptr, nullptr, nullptr));
    CALL(h, ljmd_batch_steps(h, 3, 0, nullptr, nullptr, nullptr, nullptr));
    CALL(h, ljmd_batch_steps(h, 0, 0, nullptr, nullptr, nullptr, nullptr));
    CALL(h, ljmd_batch_set_precision(h, LJMD_PRECISION_FP32_FORCE));
    CALL(h, ljmd_batch_set_precision(h, LJMD_PRECISION_FP64));
    CALL(h, ljmd_batch_set_tail_corrections(h, 0));
    CALL(h, ljmd_batch_get_state(h, x, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0));
    t.destroy();
}

// compute_forces, kinetic_energy and ljmd_batch_steps with neither, either and both accumulators; the handle comes with
// state and leaves with both accumulators off
void stepping(Batch &t, const char *mode_name)
{
    ljmd_batch_t *h = t.h;
    std::printf("-- stepping, %s: no accumulator --\n", mode_name);
    t.forces();
    t.kinetic();
    t.steps(12, 4);
    t.steps(6, 0);
    std::printf("-- stepping, %s: g(r) every 3 --\n", mode_name);
    CALL(h, ljmd_batch_rdf_configure(h, 16, nullptr, 3));
    t.steps(6, 0);
    t.steps(12, 6);
    t.rdf_read(16);
    CALL(h, ljmd_batch_rdf_configure(h, 0, nullptr, 0));
    std::printf("-- stepping, %s: MSD / VACF every 2, max_lag 4, stride 2 --\n", mode_name);
    CALL(h, ljmd_batch_tcf_configure(h, 4, 2, 2));
    t.steps(6, 0);
    t.steps(12, 4);                          // the numbering carries over
    t.tcf_read(4);
    t.set_state();                           // a new trajectory: numbering back to 0, counts stay
    t.forces();
    t.steps(6, 3);
    t.tcf_read(4);
    std::printf("-- stepping, %s: g(r) every 3 and MSD / VACF every 2 --\n", mode_name);
    CALL(h, ljmd_batch_rdf_configure(h, 16, nullptr, 3));
    t.steps(6, 0);
    t.steps(12, 12);
    t.steps(5, 0);
    t.steps(3, 0);
    t.rdf_read(16);
    t.tcf_read(4);
    std::printf("-- stand-alone accumulate, read, reset, %s --\n", mode_name);
    CALL(h, ljmd_batch_rdf_accumulate(h));
    CALL(h, ljmd_batch_tcf_accumulate(h));
    CALL(h, ljmd_batch_tcf_accumulate(h));
    t.rdf_read(16);
    t.tcf_read(4);
    CALL(h, ljmd_batch_rdf_reset(h));
    CALL(h, ljmd_batch_tcf_reset(h));
    t.rdf_read(16);
    t.tcf_read(4);
    CALL(h, ljmd_batch_tcf_accumulate(h));   // snapshot 0 again: stored, nothing live
    CALL(h, ljmd_batch_tcf_accumulate(h));
    t.tcf_read(4);
    CALL(h, ljmd_batch_rdf_configure(h, 0, nullptr, 0));
    CALL(h, ljmd_batch_tcf_configure(h, 0, 1, 0));
    CALL(h, ljmd_batch_rdf_read(h, nullptr, nullptr));
    CALL(h, ljmd_batch_tcf_read(h, nullptr, nullptr, nullptr, nullptr));
    t.steps(6, 0);
}

void heterogeneous(const char *group_streams)
{
    if (group_streams) setenv("LJMD_BATCH_GROUP_STREAMS", group_streams, 1);
    else unsetenv("LJMD_BATCH_GROUP_STREAMS");
    std::printf("== heterogeneous handle, LJMD_BATCH_GROUP_STREAMS %s ==\n", group_streams ? group_streams : "unset");
    Batch t;
    create_heterogeneous(&t, kHetB);
    unsetenv("LJMD_BATCH_GROUP_STREAMS");
    t.set_state();
    stepping(t, "fp64");
    CALL(t.h, ljmd_batch_set_precision(t.h, LJMD_PRECISION_FP64_REPRODUCIBLE));
    t.steps(6, 0);                           // the precision change dropped the state
    t.set_state();
    if (group_streams) {                     // one stream: the short form
        t.forces();
        t.steps(12, 4);
    } else {
        stepping(t, "reproducible");
    }
    CALL(t.h, ljmd_batch_set_precision(t.h, LJMD_PRECISION_FP64_REPRODUCIBLE));
    CALL(t.h, ljmd_batch_set_precision(t.h, LJMD_PRECISION_FP64));
    t.set_state();
    t.forces();
    t.steps(12, 0);                          // the fp64 plan again
    t.destroy();
}

// enough replicas of n = 4000 that the one group's launches come in chunks (256 per launch in the reproducible mode)
void many_replicas()
{
    section("many-replica handle: 260 x 4000");
    Batch t;
    CALL(nullptr, ljmd_batch_create(&t.h, 260, 4000, 20.0, 0.005, 2.5, LJMD_PRECISION_FP64, 0));
    t.adopt(260);
    ljmd_batch_t *h = t.h;
    CALL(h, ljmd_batch_rdf_configure(h, 32, nullptr, 2));
    t.set_state();
    t.forces();
    t.steps(8, 4);
    CALL(h, ljmd_batch_set_precision(h, LJMD_PRECISION_FP64_REPRODUCIBLE));
    t.set_state();
    t.forces();
    t.kinetic();
    t.steps(4, 2);
    CALL(h, ljmd_batch_rdf_accumulate(h));
    t.rdf_read(32);
    t.destroy();
}

// what a poisoned handle answers, then the recovery
void poisoned_then_recovered(Batch &t)
{
    ljmd_batch_t *h = t.h;
    t.steps(6, 0);
    t.forces();
    t.kinetic();
    CALL(h, ljmd_batch_rdf_accumulate(h));
    CALL(h, ljmd_batch_tcf_accumulate(h));
    t.rdf_read(16);                          // the reads do not look at the poison
    t.tcf_read(4);
    CALL(h, ljmd_batch_set_accel(h, t.z(), t.z(), t.z()));
    t.set_state();
    t.forces();
    t.steps(6, 0);
}

void injected_failures()
{
    section("injected launch failures");
    Batch t;
    create_heterogeneous(&t, 4);             // three groups, on streams of their own
    ljmd_batch_t *h = t.h;
    CALL(h, ljmd_batch_rdf_configure(h, 16, nullptr, 3));
    CALL(h, ljmd_batch_tcf_configure(h, 4, 2, 2));
    t.set_state();
    t.forces();
    std::printf("-- launch_batch: 3rd launch of ljmd_batch_steps --\n");
    g_fail_in[kBatch] = 3;
    t.steps(6, 0);
    poisoned_then_recovered(t);
    std::printf("-- launch_batch: 2nd launch of ljmd_batch_compute_forces --\n");
    g_fail_in[kBatch] = 2;
    t.forces();
    poisoned_then_recovered(t);
    std::printf("-- launch_batch: 1st launch of ljmd_batch_kinetic_energy --\n");
    g_fail_in[kBatch] = 1;
    t.kinetic();
    poisoned_then_recovered(t);
    std::printf("-- launch_batch_rdf: 2nd launch, in ljmd_batch_steps --\n");
    g_fail_in[kRdf] = 2;
    t.steps(6, 0);
    poisoned_then_recovered(t);
    std::printf("-- launch_batch_rdf: 1st launch, in ljmd_batch_rdf_accumulate --\n");
    g_fail_in[kRdf] = 1;
    CALL(h, ljmd_batch_rdf_accumulate(h));
    poisoned_then_recovered(t);
    std::printf("-- launch_batch_tcf: 2nd launch, in ljmd_batch_steps --\n");
    g_fail_in[kTcf] = 2;
    t.steps(6, 0);
    poisoned_then_recovered(t);
    std::printf("-- launch_batch_tcf: 1st launch, in ljmd_batch_tcf_accumulate --\n");
    g_fail_in[kTcf] = 1;
    CALL(h, ljmd_batch_tcf_accumulate(h));
    poisoned_then_recovered(t);
    std::printf("-- a set MSD / VACF range word: the reads fail until the reset, stepping goes on --\n");
    g_flag_tcf = 3;
    CALL(h, ljmd_batch_tcf_accumulate(h));
    t.tcf_read(4);
    t.steps(6, 0);
    CALL(h, ljmd_batch_tcf_reset(h));
    t.tcf_read(4);
    std::printf("-- launch_batch_fixed: 3rd launch of ljmd_batch_steps --\n");
    CALL(h, ljmd_batch_set_precision(h, LJMD_PRECISION_FP64_REPRODUCIBLE));
    t.set_state();
    t.forces();
    g_fail_in[kFixed] = 3;
    t.steps(6, 3);
    poisoned_then_recovered(t);
    std::printf("-- launch_batch_fixed: 1st launch of ljmd_batch_compute_forces --\n");
    g_fail_in[kFixed] = 1;
    t.forces();
    poisoned_then_recovered(t);
    std::printf("-- a set range word of the reproducible mode: replica 2 --\n");
    g_flag_fixed = 2;
    t.steps(6, 0);
    poisoned_then_recovered(t);
    g_flag_fixed = 1;
    t.kinetic();
    poisoned_then_recovered(t);
    t.destroy();
}

}  // namespace

int main()
{
    setenv("FAKEHIP_DEVICES", "1", 1);
    std::setvbuf(stdout, nullptr, _IOLBF, 0);
    guards_without_handle();
    guards_with_handle();
    heterogeneous(nullptr);
    heterogeneous("0");
    many_replicas();
    injected_failures();
    std::printf("done\n");
    return 0;
}
