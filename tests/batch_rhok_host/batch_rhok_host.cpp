// batch_rhok_host.cpp -- TEST INFRASTRUCTURE: the host code of the batch engine's density modes
// (csrc/ljmd_rhok_batch.cpp) and of the step loop that serves it, without a GPU.  Linked from the batch host files,
// ljmd_rhok_batch.cpp, ljmd_common.cpp, the fake HIP runtime (tests/fakehip) and its own definitions of the launchers.
// The density modes launcher carries out the kernel's meaning on the host with ljmd_rhok_arith.h -- the fake runtime's
// device memory is host memory -- and the step launcher moves every r by an exactly representable amount per step, so
// that the C ABI can be checked against a brute-force loop over replicas, modes and particles: configure, accumulate,
// `every` inside ljmd_batch_steps, read, read_exact, reset, the full series, the range word, an injected launch failure,
// release and destroy, every guard's code and message, the arguments of every launch and the byte counts of configure.
// hipMalloc and hipFree of the fake runtime are wrapped at link time (-Wl,--wrap) so that the program sees the
// allocations.  It checks itself, prints one line per check that fails and "batch_rhok_host: ok" when none did.
// tests/test_batch_rhok_host.py runs it under ASan and UBSan.
#include "ljmd.h"
#include "ljmd_batch_host.h"
#include "ljmd_batch_rhok.h"
#include "ljmd_rhok_arith.h"

#include <cmath>
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
std::vector<size_t> g_allocs;              // byte counts of the hipMalloc calls, in order

void check(bool ok, const char *what)
{
    if (ok) return;
    ++g_failures;
    std::printf("FAILED: %s\n", what);
}

// one recorded launch: kind 'B' steps / forces, 'R' g(r), 'T' MSD / VACF, 'K' density modes
struct Launch {
    char kind;
    int g0, n_max, n_blocks;
    hipStream_t stream;
    int step0, nsteps;                     // 'B'
    int64_t row;                           // 'K'
    int waves;                             // 'K'
    bool operator==(const Launch &o) const
    {
        return kind == o.kind && g0 == o.g0 && n_max == o.n_max && n_blocks == o.n_blocks && stream == o.stream &&
               step0 == o.step0 && nsteps == o.nsteps;
    }
};
std::vector<Launch> g_log;
int g_fail_rhok = 0;                       // k > 0: the k-th density modes launch from now returns hipErrorLaunchFailure

// Q(t) = RNE(t 2^64) as an integer; |t| <= 2
__int128 Q(double t) { return (__int128)std::rint(t * 0x1p64); }

bool words_are(const int64_t *w, __int128 x)
{
    return (uint64_t)w[0] == (uint64_t)x && (uint64_t)w[1] == (uint64_t)(x >> 64) && w[2] == (x < 0 ? -1 : 0);
}

}  // namespace

extern "C" {

hipError_t __wrap_hipMalloc(void **p, size_t n)
{
    g_allocs.push_back(n);
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

// the step kernel's stand-in: r of particle i, axis c moves by (c + 1) (i % 7 + 1) 2^-10 per step -- exact in doubles
hipError_t launch_batch(const BatchArgs &a, int n_max, int n_blocks, hipStream_t s)
{
    g_log.push_back({'B', a.g0, n_max, n_blocks, s, a.step0, a.nsteps, 0, 0});
    if (a.mode != kModeSteps) return hipSuccess;
    for (int k = 0; k < n_blocks; ++k) {
        const BatchReplica &rp = a.rep[a.g0 + k];
        for (int c = 0; c < 3; ++c)
            for (int i = 0; i < rp.n; ++i)
                a.state[(size_t)c * a.plane + rp.off + i] += a.nsteps * (c + 1) * (i % 7 + 1) * 0x1p-10;
    }
    return hipSuccess;
}

hipError_t launch_batch_fixed(const BatchFixedArgs &a, int n_max, int n_blocks, hipStream_t s)
{
    return launch_batch(a.b, n_max, n_blocks, s);
}

hipError_t launch_batch_rdf(const BatchRdfArgs &a, int n_max, int n_blocks, hipStream_t s)
{
    g_log.push_back({'R', a.g0, n_max, n_blocks, s, 0, 0, 0, 0});
    return hipSuccess;
}

hipError_t launch_batch_tcf(const BatchTcfArgs &a, int n_max, int n_blocks, hipStream_t s)
{
    g_log.push_back({'T', a.g0, n_max, n_blocks, s, 0, 0, 0, 0});
    return hipSuccess;
}

// the meaning of batch_rhok_kernel, replica by replica and mode by mode: the two-part accumulators of a lane
hipError_t launch_batch_rhok(const BatchRhokArgs &a, int n_blocks, int waves, hipStream_t s)
{
    g_log.push_back({'K', a.g0, 0, n_blocks, s, 0, 0, a.row, waves});
    check(batch_rhok_ok(a, n_blocks, waves), "a density modes launch passes the launcher's own check");
    if (g_fail_rhok > 0 && --g_fail_rhok == 0) return hipErrorLaunchFailure;
    for (int k = 0; k < n_blocks; ++k) {
        const BatchReplica &rp = a.rep[a.g0 + k];
        for (int m = 0; m < a.n_modes; ++m) {
            const double nx = (double)a.modes[3 * m], ny = (double)a.modes[3 * m + 1], nz = (double)a.modes[3 * m + 2];
            long long re_hi = 0, re_lo = 0, im_hi = 0, im_lo = 0;
            for (int i = 0; i < rp.n; ++i) {
                const double tx = ljmdk::rhok_turns(a.r[rp.off + i], rp.L);
                const double ty = ljmdk::rhok_turns(a.r[a.plane + rp.off + i], rp.L);
                const double tz = ljmdk::rhok_turns(a.r[2 * a.plane + rp.off + i], rp.L);
                double C, S;
                ljmdk::rhok_term(nx, ny, nz, tx, ty, tz, C, S);
                const bool oob = ljmdk::rhok_out_of_range(C, S);
                if (oob) a.range[rp.b] = 1;
                long long hi, lo;
                ljmdk::rhok_fixed_parts(oob ? 0.0 : C, hi, lo);
                re_hi += hi; re_lo += lo;
                ljmdk::rhok_fixed_parts(oob ? 0.0 : S, hi, lo);
                im_hi += hi; im_lo += lo;
            }
            uint64_t *dst = a.words + (((size_t)a.row * a.B + (size_t)rp.b) * (size_t)a.n_modes + (size_t)m) * kBatchRhokRowWords;
            uint64_t q[3];
            ljmdk::from128(q, (__int128)re_hi * ((__int128)1 << 32) + (__int128)re_lo);
            dst[0] = q[0]; dst[1] = q[1]; dst[2] = q[2];
            ljmdk::from128(q, (__int128)im_hi * ((__int128)1 << 32) + (__int128)im_lo);
            dst[3] = q[0]; dst[4] = q[1]; dst[5] = q[2];
        }
    }
    return hipSuccess;
}

}  // namespace ljmdb

namespace {

using namespace ljmdb;

bool message_has(const ljmd_batch_t *h, const char *text) { return std::strstr(ljmd_batch_last_error(h), text) != nullptr; }
bool message_is(const ljmd_batch_t *h, const std::string &text) { return text == ljmd_batch_last_error(h); }

int steps(ljmd_batch_t *h, int n) { return ljmd_batch_steps(h, n, 1, nullptr, nullptr, nullptr, nullptr); }

std::vector<Launch> only(char kind)
{
    std::vector<Launch> out;
    for (const Launch &l : g_log)
        if (l.kind == kind) out.push_back(l);
    return out;
}

constexpr int kB = 3;
const int32_t kN[kB] = {5, 130, 8};               // two kernel classes: two groups
const double kL[kB] = {6.0, 12.0, 6.0}, kDt[kB] = {0.005, 0.005, 0.005}, kRc[kB] = {2.5, 2.5, 2.5};
constexpr int kModes = 7;
const int32_t kModeList[kModes * 3] = {0, 0, 0, 1, 0, 0, -1, 0, 0, 3, -2, 7, 1023, -1023, 1023, 1, 0, 0, 0, 4, 0};

ljmd_batch_t *create()
{
    ljmd_batch_t *h = nullptr;
    check(ljmd_batch_create_per_replica(&h, kB, kN, kL, kDt, kRc, LJMD_PRECISION_FP64, 0) == LJMD_OK && h, "create");
    return h;
}

// positions on a grid of 2^-4 inside the box: every later r is a multiple of 2^-10
int set_grid_state(ljmd_batch_t *h, int shift)
{
    std::vector<double> x(h->total), y(h->total), z(h->total), zero(h->total, 0.0);
    for (size_t b = 0; b < h->B; ++b)
        for (int i = 0; i < h->rep[b].n; ++i) {
            const size_t k = (size_t)h->offsets[b] + i;
            x[k] = ((i + shift) % 16) * 0x1p-4;
            y[k] = ((i / 16 + shift) % 16) * 0x1p-4;
            z[k] = ((int)b % 16) * 0x1p-4;
        }
    return ljmd_batch_set_state(h, x.data(), y.data(), z.data(), zero.data(), zero.data(), zero.data());
}

// particle i at (i % 4) L / 4 along x and 0 elsewhere: exp(i k . r) of mode (1, 0, 0) is a power of i exactly
int set_quarter_state(ljmd_batch_t *h)
{
    std::vector<double> x(h->total), zero(h->total, 0.0);
    for (size_t b = 0; b < h->B; ++b)
        for (int i = 0; i < h->rep[b].n; ++i) x[(size_t)h->offsets[b] + i] = (i % 4) * (0.25 * h->rep[b].L);
    return ljmd_batch_set_state(h, x.data(), zero.data(), zero.data(), zero.data(), zero.data(), zero.data());
}

// the resident r of every replica: [3][total]
std::vector<double> snapshot(ljmd_batch_t *h)
{
    std::vector<double> r(3 * h->total);
    check(ljmd_batch_get_state(h, r.data(), r.data() + h->total, r.data() + 2 * h->total, nullptr, nullptr, nullptr, nullptr,
                               nullptr, nullptr, nullptr, nullptr, nullptr) == LJMD_OK, "get_state");
    return r;
}

// the definition by brute force: [B][n_modes][2] integers of one snapshot; a term that is not finite adds nothing
std::vector<__int128> brute(const ljmd_batch_t *h, const std::vector<double> &r, const int32_t *modes, int n_modes,
                            std::vector<int> *flags = nullptr)
{
    std::vector<__int128> out((size_t)h->B * n_modes * 2, 0);
    if (flags) flags->assign(h->B, 0);
    for (size_t b = 0; b < h->B; ++b)
        for (int m = 0; m < n_modes; ++m)
            for (int i = 0; i < h->rep[b].n; ++i) {
                const size_t k = (size_t)h->offsets[b] + i;
                const double L = h->rep[b].L;
                double C, S;
                ljmdk::rhok_term((double)modes[3 * m], (double)modes[3 * m + 1], (double)modes[3 * m + 2], ljmdk::rhok_turns(r[k], L),
                                 ljmdk::rhok_turns(r[h->total + k], L), ljmdk::rhok_turns(r[2 * h->total + k], L), C, S);
                if (!std::isfinite(C) || !std::isfinite(S)) {
                    if (flags) (*flags)[b] = 1;
                    continue;
                }
                out[(b * n_modes + m) * 2] += Q(C);
                out[(b * n_modes + m) * 2 + 1] += Q(S);
            }
    return out;
}

// both reads against the expected rows; `expect` is the return code of both
void compare(ljmd_batch_t *h, const std::vector<std::vector<__int128>> &rows, int n_modes, const char *what)
{
    const size_t per = (size_t)kB * n_modes * 2;
    std::vector<int64_t> words(rows.size() * per * 3 + 3, 99);
    std::vector<double> rho(rows.size() * per + 1, -7.0);
    int64_t snaps = -1, snaps2 = -1;
    check(ljmd_batch_rhok_read_exact(h, words.data(), &snaps) == LJMD_OK, what);
    check(ljmd_batch_rhok_read(h, rho.data(), &snaps2) == LJMD_OK, what);
    bool ok = snaps == (int64_t)rows.size() && snaps2 == snaps && words[rows.size() * per * 3] == 99 && rho[rows.size() * per] == -7.0;
    for (size_t s = 0; s < rows.size(); ++s)
        for (size_t k = 0; k < per; ++k) {
            const int64_t *w = words.data() + (s * per + k) * 3;
            ok = ok && words_are(w, rows[s][k]);
            const uint64_t u[3] = {(uint64_t)w[0], (uint64_t)w[1], (uint64_t)w[2]};
            ok = ok && rho[s * per + k] == ljmdk::fixed_to_double(u);
        }
    check(ok, what);
}

// 1. the guards: codes and messages, in the header's order
void guards()
{
    const std::string cfg = "ljmd_batch_rhok_configure: ";
    check(ljmd_batch_rhok_configure(nullptr, -1, nullptr, -1, -1) == LJMD_ERR_INVALID_ARG && message_is(nullptr, cfg + "NULL handle"),
          "configure: NULL handle first");
    check(ljmd_batch_rhok_accumulate(nullptr) == LJMD_ERR_INVALID_ARG && ljmd_batch_rhok_reset(nullptr) == LJMD_ERR_INVALID_ARG &&
              ljmd_batch_rhok_read(nullptr, nullptr, nullptr) == LJMD_ERR_INVALID_ARG &&
              ljmd_batch_rhok_profile_read(nullptr, nullptr) == LJMD_ERR_INVALID_ARG &&
              ljmd_batch_rhok_read_exact(nullptr, nullptr, nullptr) == LJMD_ERR_INVALID_ARG &&
              message_is(nullptr, "ljmd_batch_rhok_read_exact: NULL handle"), "the other calls: NULL handle");
    ljmd_batch_t *h = create();
    if (!h) return;
    const long base = g_live;
    std::vector<int32_t> many((size_t)3 * 4097, 1);
    int32_t bad_lo[6] = {1, 2, 3, 0, -1024, 0}, bad_hi[6] = {1, 2, 3, 0, 0, 1024};
    struct Case { int n_modes; const int32_t *modes; int max_snapshots, every; std::string msg; };
    const Case cases[] = {
        {-1, nullptr, -1, -1, cfg + "max_snapshots = -1 outside 1..262144 (0 switches the density modes off)"},
        {-1, nullptr, 262145, -1, cfg + "max_snapshots = 262145 outside 1..262144 (0 switches the density modes off)"},
        {-1, nullptr, 0, -1, cfg + "every must be >= 0"},
        {0, nullptr, 2, 0, cfg + "n_modes = 0 outside 1..4096"},
        {4097, many.data(), 2, 0, cfg + "n_modes = 4097 outside 1..4096"},
        {2, nullptr, 2, 0, cfg + "modes is NULL"},
        {2, bad_lo, 262144, 0, cfg + "mode 1 = (0, -1024, 0): an index outside -1023..1023"},
        {2, bad_hi, 262144, 0, cfg + "mode 1 = (0, 0, 1024): an index outside -1023..1023"},
        {4096, many.data(), 1366, 0, cfg + "max_snapshots * B * n_modes = 16785408 above 16777216"},
    };
    for (const Case &c : cases)
        check(ljmd_batch_rhok_configure(h, c.n_modes, c.modes, c.max_snapshots, c.every) == LJMD_ERR_INVALID_ARG && message_is(h, c.msg),
              c.msg.c_str());
    check(g_live == base && h->rhok.max_snapshots == 0 && !h->rhok.release && !h->rhok.acc.enqueue,
          "the refused calls allocate nothing and leave the handle's entries empty");
    const char *first = "call ljmd_batch_rhok_configure first";
    check(ljmd_batch_rhok_accumulate(h) == LJMD_ERR_STATE && message_is(h, std::string("ljmd_batch_rhok_accumulate: ") + first),
          "accumulate before configure");
    check(ljmd_batch_rhok_read(h, nullptr, nullptr) == LJMD_ERR_STATE && ljmd_batch_rhok_read_exact(h, nullptr, nullptr) == LJMD_ERR_STATE &&
              ljmd_batch_rhok_profile_read(h, nullptr) == LJMD_ERR_STATE && ljmd_batch_rhok_reset(h) == LJMD_ERR_STATE &&
              message_is(h, std::string("ljmd_batch_rhok_reset: ") + first), "read, read_exact, profile_read, reset before configure");

    // the entry guard: the density modes are asked behind van Hove and before the state
    const unsigned all = kNeedRhok | kNeedState | kNeedSound;
    check(enter(h, "who", all | kNeedVanhove) == LJMD_ERR_STATE && message_has(h, "call ljmd_batch_vanhove_configure first"),
          "van Hove is asked before them");
    check(enter(h, "who", all) == LJMD_ERR_STATE && message_is(h, std::string("who: ") + first), "then the density modes");

    // configure: three buffers, their byte counts in size_t, in this order
    g_allocs.clear();
    check(ljmd_batch_rhok_configure(h, kModes, kModeList, 5, 0) == LJMD_OK && g_live == base + 3, "configure allocates three buffers");
    const std::vector<size_t> want = {(size_t)5 * kB * kModes * 48, (size_t)kModes * 12, (size_t)kB * 4};
    check(g_allocs == want, "the series, the mode list, the range words");
    check(h->rhok.n_modes == kModes && h->rhok.waves == kBatchRhokWaves && h->rhok.count == 0 &&
              std::memcmp(h->rhok.d_modes, kModeList, sizeof kModeList) == 0, "the list is on the device, the built-in wave count");
    check(enter(h, "who", all) == LJMD_ERR_STATE && message_has(h, "no state has been set"), "then the state");
    check(ljmd_batch_rhok_configure(h, 0, kModeList, 3, 0) == LJMD_ERR_INVALID_ARG && h->rhok.max_snapshots == 5 && g_live == base + 3,
          "a failed guard keeps the earlier configuration");
    check(ljmd_batch_rhok_accumulate(h) == LJMD_ERR_STATE && message_has(h, "no state has been set"), "accumulate before a state");
    check(set_grid_state(h, 0) == LJMD_OK, "set_state");
    h->poisoned = true;
    check(ljmd_batch_rhok_accumulate(h) == LJMD_ERR_STATE && message_has(h, "poisoned"), "accumulate on a poisoned handle");
    int64_t snaps = -1;
    double ms = -1.0;
    check(ljmd_batch_rhok_read(h, nullptr, &snaps) == LJMD_OK && snaps == 0 && ljmd_batch_rhok_profile_read(h, &ms) == LJMD_OK && ms == 0.0,
          "a poisoned handle may still be read");
    h->poisoned = false;
    g_log.clear();
    check(ljmd_batch_rhok_accumulate(h) == LJMD_OK && only('K').size() == 2 && g_log.size() == 2 && h->rhok.count == 1,
          "accumulate needs no accelerations: one launch per group");

    // the wave count of the launches: the knob is read by configure, and only 2, 4 and 8 are taken
    for (const char *v : {"8", "2", "3", "4"}) {
        setenv("LJMD_BATCH_RHOK_WAVES", v, 1);
        check(ljmd_batch_rhok_configure(h, kModes, kModeList, 2, 0) == LJMD_OK, "reconfigure");
        g_log.clear();
        const int expect = std::atoi(v) == 3 ? kBatchRhokWaves : std::atoi(v);
        check(ljmd_batch_rhok_accumulate(h) == LJMD_OK && g_log.size() == 2 && g_log[0].waves == expect && g_log[1].waves == expect,
              "LJMD_BATCH_RHOK_WAVES = 2, 4 or 8 reaches the launches; anything else is the built-in choice");
    }
    unsetenv("LJMD_BATCH_RHOK_WAVES");

    // a failed allocation: everything released, the feature off, the message naming buffer and bytes
    g_fail_alloc_of = (size_t)kModes * 12;
    check(ljmd_batch_rhok_configure(h, kModes, kModeList, 4, 0) == LJMD_ERR_ALLOC &&
              message_is(h, cfg + "cannot allocate 84 bytes of the mode list") && g_live == base && h->rhok.max_snapshots == 0 &&
              !h->rhok.release, "a failed allocation: LJMD_ERR_ALLOC with the feature off");
    g_fail_alloc_of = 0;
    check(ljmd_batch_rhok_accumulate(h) == LJMD_ERR_STATE, "off after it");
    check(ljmd_batch_rhok_configure(h, kModes, kModeList, 4, 0) == LJMD_OK && g_live == base + 3, "configure again");
    check(ljmd_batch_rhok_configure(h, -5, nullptr, 0, 0) == LJMD_OK && g_live == base && !h->rhok.release,
          "configure(max_snapshots = 0) frees it, whatever the mode arguments");
    check(ljmd_batch_rhok_configure(h, kModes, kModeList, 4, 0) == LJMD_OK, "once more: destroyed while configured");
    ljmd_batch_destroy(h);
    check(g_live == 0, "destroy frees everything");
}

// 2. accumulate against the brute-force loop and against values known exactly; the full series; reset
void against_brute_force()
{
    ljmd_batch_t *h = create();
    if (!h) return;
    check(ljmd_batch_rhok_configure(h, kModes, kModeList, 3, 0) == LJMD_OK, "configure");
    std::vector<std::vector<__int128>> rows;
    // positions at quarters of the box along x: mode (1, 0, 0) sums powers of i, (0, 4, 0) and (0, 0, 0) count particles
    check(set_quarter_state(h) == LJMD_OK && ljmd_batch_rhok_accumulate(h) == LJMD_OK, "the quarter state");
    rows.push_back(brute(h, snapshot(h), kModeList, kModes));
    const __int128 one = (__int128)1 << 64;
    bool ok = true;
    for (int b = 0; b < kB; ++b) {
        int c[4] = {0, 0, 0, 0};
        for (int i = 0; i < kN[b]; ++i) ++c[i % 4];
        const __int128 *w = rows[0].data() + (size_t)b * kModes * 2;
        ok = ok && w[0] == kN[b] * one && w[1] == 0;                                   // (0, 0, 0)
        ok = ok && w[2] == (c[0] - c[2]) * one && w[3] == (c[1] - c[3]) * one;         // (1, 0, 0): 1, i, -1, -i
        ok = ok && w[4] == w[2] && w[5] == -w[3];                                      // (-1, 0, 0): the conjugate
        ok = ok && w[10] == w[2] && w[11] == w[3];                                     // the duplicate
        ok = ok && w[12] == kN[b] * one && w[13] == 0;                                 // (0, 4, 0) at y = 0
    }
    check(ok, "the brute-force loop gives the values known exactly at quarters of the box");
    compare(h, rows, kModes, "one snapshot equals the brute-force loop");
    for (int s = 1; s < 3; ++s) {
        check(set_grid_state(h, s) == LJMD_OK && ljmd_batch_compute_forces(h, nullptr, nullptr, nullptr) == LJMD_OK && steps(h, 2 + s) == LJMD_OK,
              "another state");
        g_log.clear();
        check(ljmd_batch_rhok_accumulate(h) == LJMD_OK, "accumulate");
        bool lok = g_log.size() == 2;
        for (size_t g = 0; g < g_log.size(); ++g)
            lok = lok && g_log[g].kind == 'K' && g_log[g].stream == h->stream && g_log[g].g0 == (int)h->groups[g].first &&
                  g_log[g].n_blocks == (int)h->groups[g].count && g_log[g].row == s && g_log[g].waves == kBatchRhokWaves;
        check(lok, "one launch per group on the handle's stream, writing the next row");
        rows.push_back(brute(h, snapshot(h), kModeList, kModes));
    }
    check(rows[1] != rows[2] && rows[0] != rows[1], "the snapshots differ");
    compare(h, rows, kModes, "three snapshots equal the brute-force loop");
    g_log.clear();
    check(ljmd_batch_rhok_accumulate(h) == LJMD_ERR_STATE && g_log.empty() &&
              message_is(h, "ljmd_batch_rhok_accumulate: the density modes series is full: 3 of 3 snapshots taken, 1 more do not fit "
                            "(read it, then ljmd_batch_rhok_reset)"), "the full series refuses before anything is launched");
    compare(h, rows, kModes, "... and stays what it is");
    check(ljmd_batch_rhok_read(h, nullptr, nullptr) == LJMD_OK && ljmd_batch_rhok_read_exact(h, nullptr, nullptr) == LJMD_OK,
          "every pointer may be NULL");
    check(ljmd_batch_rhok_reset(h) == LJMD_OK && h->rhok.count == 0, "reset");
    compare(h, {}, kModes, "reset empties the series");
    bool zero = true;
    for (size_t k = 0; k < (size_t)3 * kB * kModes * 6; ++k) zero = zero && h->rhok.d_words[k] == 0;
    check(zero, "... and zeroes it");
    check(ljmd_batch_rhok_accumulate(h) == LJMD_OK, "accumulate after reset");
    compare(h, {rows[2]}, kModes, "the first row again");
    // one mode, a list of its own: a mode's words do not depend on the list
    check(ljmd_batch_rhok_configure(h, 1, kModeList + 9, 1, 0) == LJMD_OK && ljmd_batch_rhok_accumulate(h) == LJMD_OK, "one mode");
    std::vector<__int128> alone;
    for (int b = 0; b < kB; ++b)
        for (int c = 0; c < 2; ++c) alone.push_back(rows[2][((size_t)b * kModes + 3) * 2 + c]);
    compare(h, {alone}, 1, "mode (3, -2, 7) alone has the words it has in the list");
    ljmd_batch_destroy(h);
    check(g_live == 0, "destroy frees everything");
}

// 3. `every` inside ljmd_batch_steps, beside MSD / VACF and g(r); off is off; the range word; an injected failure
void inside_steps()
{
    ljmd_batch_t *h = create();
    if (!h) return;
    check(h->groups.size() == 2 && h->concurrent, "two groups on streams of their own");
    check(set_grid_state(h, 0) == LJMD_OK && ljmd_batch_compute_forces(h, nullptr, nullptr, nullptr) == LJMD_OK, "state");
    check(ljmd_batch_rdf_configure(h, 8, nullptr, 4) == LJMD_OK && ljmd_batch_tcf_configure(h, 4, 1, 2) == LJMD_OK, "g(r), MSD / VACF");
    g_log.clear();
    check(steps(h, 12) == LJMD_OK, "steps without the density modes");
    const std::vector<Launch> before = g_log;
    check(only('K').empty() && !only('R').empty() && !only('T').empty(), "its transcript");
    auto restart = [&] {
        return ljmd_batch_tcf_reset(h) == LJMD_OK && set_grid_state(h, 0) == LJMD_OK &&
               ljmd_batch_compute_forces(h, nullptr, nullptr, nullptr) == LJMD_OK;
    };
    check(ljmd_batch_rhok_configure(h, kModes, kModeList, 6, 0) == LJMD_OK && restart(), "configure with every == 0");
    g_log.clear();
    check(steps(h, 12) == LJMD_OK && g_log == before, "every == 0: the same launches");
    check(ljmd_batch_rhok_configure(h, 0, nullptr, 0, 0) == LJMD_OK && restart(), "configure(0)");
    g_log.clear();
    check(steps(h, 12) == LJMD_OK && g_log == before, "switched off: the same launches");

    // every = 3 beside 4 (g(r)) and 2 (MSD / VACF): a launch ends at the multiples of any of them
    check(ljmd_batch_rhok_configure(h, kModes, kModeList, 8, 3) == LJMD_OK && restart(), "configure(every = 3)");
    std::vector<std::vector<__int128>> rows;
    rows.push_back(brute(h, snapshot(h), kModeList, kModes));
    check(ljmd_batch_rhok_accumulate(h) == LJMD_OK, "snapshot 0 by hand");
    g_log.clear();
    check(steps(h, 8) == LJMD_ERR_INVALID_ARG && g_log.empty() &&
              message_is(h, "ljmd_batch_steps: nsteps 8 is not a multiple of the density modes interval 3 (ljmd_batch_rhok_configure: every)"),
          "nsteps % every != 0 is refused before anything launches");
    check(steps(h, 9) == LJMD_ERR_INVALID_ARG && message_has(h, "g(r) interval 4"), "g(r) is asked before it");
    check(steps(h, 24) == LJMD_ERR_STATE && g_log.empty() &&
              message_is(h, "ljmd_batch_steps: the density modes series is full: 1 of 8 snapshots taken, 8 more do not fit "
                            "(read it, then ljmd_batch_rhok_reset)"), "the room check comes before anything launches");
    check(steps(h, 12) == LJMD_OK && h->rhok.count == 5, "steps(12): four snapshots, counted once each");
    int32_t launches = 0;
    check(ljmd_batch_profile_read(h, nullptr, &launches) == LJMD_OK && launches == (int32_t)g_log.size(), "profile_read counts them");
    for (const BatchGroup &g : h->groups) {
        std::vector<Launch> mine;
        for (const Launch &l : g_log)
            if (l.g0 >= (int)g.first && l.g0 < (int)(g.first + g.count)) mine.push_back(l);
        int k = 0, ends = 0;
        bool ok = !mine.empty();
        for (size_t i = 0; i < mine.size(); ++i) {
            ok = ok && mine[i].stream == g.stream && g.stream != h->stream;
            if (mine[i].kind == 'B') {
                const int end = mine[i].step0 + mine[i].nsteps;
                ok = ok && (end % 3 == 0 || end % 2 == 0);
                ++ends;
            }
            if (mine[i].kind != 'K') continue;
            // the last launch of its step: behind the step launch that ends at 3 (k + 1) and the other accumulators'
            size_t prev = i - 1;
            while (prev > 0 && (mine[prev].kind == 'R' || mine[prev].kind == 'T')) --prev;
            ok = ok && i > 0 && mine[prev].kind == 'B' && mine[prev].step0 + mine[prev].nsteps == 3 * (k + 1) &&
                 (i + 1 == mine.size() || mine[i + 1].kind == 'B') && mine[i].g0 == (int)g.first && mine[i].n_blocks == (int)g.count &&
                 mine[i].row == 1 + k;
            ++k;
        }
        check(ok && k == 4 && ends == 8, "a group's density modes launches end its steps 3, 6, 9, 12 on its own stream; cuts at 2 3 4 6 8 9 10 12");
    }
    // the snapshots inside steps are r0 + 3 k steps of the stand-in: a second handle stopped there gives the states
    {
        ljmd_batch_t *m = create();
        if (m) {
            check(set_grid_state(m, 0) == LJMD_OK && ljmd_batch_compute_forces(m, nullptr, nullptr, nullptr) == LJMD_OK, "the manual route");
            for (int k = 0; k < 4; ++k) {
                check(steps(m, 3) == LJMD_OK, "steps(3)");
                rows.push_back(brute(m, snapshot(m), kModeList, kModes));
            }
            ljmd_batch_destroy(m);
        }
        compare(h, rows, kModes, "every = 3 inside steps equals the brute-force loop on the states of a run stopped there");
    }

    // the sticky range word: the lowest replica is named, no poison, the words are delivered, reset clears it
    {
        check(ljmd_batch_rhok_reset(h) == LJMD_OK, "reset");
        h->d_state[(size_t)h->offsets[2] + 1] = std::nan("");                          // x of particle 1 of replica 2
        h->d_state[h->total + (size_t)h->offsets[1] + 7] = INFINITY;                    // y of particle 7 of replica 1
        check(ljmd_batch_rhok_accumulate(h) == LJMD_OK, "two replicas with a coordinate that is not finite");
        std::vector<int> flags;
        const std::vector<__int128> want = brute(h, snapshot(h), kModeList, kModes, &flags);
        check(flags == std::vector<int>({0, 1, 1}) && h->rhok.d_range[0] == 0 && h->rhok.d_range[1] == 1 && h->rhok.d_range[2] == 1,
              "the range words of replicas 1 and 2 are set");
        std::vector<int64_t> words((size_t)kB * kModes * 6, 99);
        std::vector<double> rho((size_t)kB * kModes * 2, -7.0);
        int64_t n_snap = -1;
        check(ljmd_batch_rhok_read_exact(h, words.data(), &n_snap) == LJMD_ERR_RANGE &&
                  message_has(h, "ljmd_batch_rhok_read_exact: replica 1: a particle's density mode terms were not finite") &&
                  message_has(h, "until ljmd_batch_rhok_reset") && !h->poisoned && n_snap == -1,
              "LJMD_ERR_RANGE names the lowest replica; no poison");
        bool ok = true;
        for (size_t k = 0; k < want.size(); ++k) ok = ok && words_are(words.data() + 3 * k, want[k]);
        check(ok && words_are(words.data() + ((size_t)1 * kModes) * 6, (__int128)(kN[1] - 1) << 64) &&
                  words_are(words.data() + ((size_t)2 * kModes) * 6, (__int128)(kN[2] - 1) << 64),
              "... with the words delivered: the particle entered as zeros, mode (0, 0, 0) included");
        check(ljmd_batch_rhok_read(h, rho.data(), nullptr) == LJMD_ERR_RANGE && rho[0] == -7.0, "read likewise, and writes nothing");
        check(steps(h, 12) == LJMD_OK, "stepping goes on");
        check(ljmd_batch_rhok_read(h, nullptr, nullptr) == LJMD_ERR_RANGE, "sticky");
        check(restart() && ljmd_batch_rhok_read(h, nullptr, nullptr) == LJMD_ERR_RANGE, "set_state keeps the word");
        check(ljmd_batch_rhok_reset(h) == LJMD_OK && ljmd_batch_rhok_read(h, nullptr, &n_snap) == LJMD_OK && n_snap == 0, "reset clears it");
    }

    // an injected launch failure: poison, then recovery through set_state
    check(restart() && steps(h, 12) == LJMD_OK && h->rhok.count == 4, "four snapshots");
    g_fail_rhok = 2;
    g_log.clear();
    check(steps(h, 12) == LJMD_ERR_HIP && message_has(h, "ljmd_batch_steps: density modes launch failed") && message_has(h, "poisoned") &&
              h->poisoned && only('K').size() == 2, "an injected launch failure poisons the handle");
    check(h->rhok.count == 4, "... and leaves the snapshot count alone");
    check(steps(h, 12) == LJMD_ERR_STATE && ljmd_batch_rhok_accumulate(h) == LJMD_ERR_STATE, "poisoned until set_state");
    int64_t n_snap = -1;
    check(ljmd_batch_rhok_read_exact(h, nullptr, &n_snap) == LJMD_OK && n_snap == 4, "... and may still be read");
    check(restart() && !h->poisoned && steps(h, 12) == LJMD_OK && h->rhok.count == 8 && h->rhok.every == 3 && h->rhok.n_modes == kModes,
          "set_state recovers and keeps configuration and series");
    ljmd_batch_destroy(h);
    check(g_live == 0, "destroy frees everything (three accumulators on)");
}

}  // namespace

int main()
{
    setenv("FAKEHIP_DEVICES", "1", 1);
    unsetenv("LJMD_BATCH_GROUP_STREAMS");
    unsetenv("LJMD_BATCH_RHOK_WAVES");
    guards();
    against_brute_force();
    inside_steps();
    if (g_failures == 0) std::printf("batch_rhok_host: ok\n");
    return g_failures == 0 ? 0 : 1;
}
