// batch_vanhove_host.cpp -- TEST INFRASTRUCTURE: the host code of the batch engine's van Hove self-correlation
// (csrc/ljmd_vanhove_batch.cpp) and of the step loop that serves it, without a GPU.  Linked from the batch host files,
// ljmd_vanhove_batch.cpp, ljmd_common.cpp, the fake HIP runtime (tests/fakehip) and its own definitions of the launchers.
// The van Hove launcher carries out the kernel's meaning on the host -- the fake runtime's device memory is host memory
// -- and the step launcher moves every ru by an exactly representable amount per step, so that the C ABI can be checked
// against a brute-force loop over stored snapshots: several (max_lag, stride, nbins), per-replica n and rmax, ring wrap, a
// new trajectory, `every` inside ljmd_batch_steps, an injected launch failure, every guard's code and message, the
// arguments of every launch and the byte counts of configure; and, for MSD / VACF beside it, that a set range word fails
// a read before anything is written.  hipMalloc and hipFree of the fake runtime are wrapped at
// link time (-Wl,--wrap) so that the program sees the allocations.  It checks itself, prints one line per check that
// fails and "batch_vanhove_host: ok" when none did.  tests/test_batch_vanhove_host.py runs it under ASan and UBSan.
#include "ljmd.h"
#include "ljmd_batch_host.h"
#include "ljmd_batch_vanhove.h"
#include "ljmd_tcf_host.h"

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

// one recorded launch: kind 'B' steps / forces, 'R' g(r), 'T' MSD / VACF, 'V' van Hove
struct Launch {
    char kind;
    int g0, n_max, n_blocks;
    hipStream_t stream;
    int step0, nsteps;                     // 'B'
    int n_live, lag_first, slot_first, store_slot;   // 'V'
    bool operator==(const Launch &o) const
    {
        return kind == o.kind && g0 == o.g0 && n_max == o.n_max && n_blocks == o.n_blocks && stream == o.stream &&
               step0 == o.step0 && nsteps == o.nsteps;
    }
};
std::vector<Launch> g_log;
int g_fail_vanhove = 0;                    // k > 0: the k-th van Hove launch from now returns hipErrorLaunchFailure
int g_tcf_flags = -1;                      // >= 0: an MSD / VACF launch sets the range word of this replica

// Q(t) = RNE(t 2^64) as an integer; |t| < 2^40
__int128 Q(double t) { return (__int128)std::rint(t * 0x1p64); }

// the per-particle term of include/ljmd.h: -> the column of H, and r2, r4 as they enter the sums
int term(const double cur[3], const double org[3], double dr, int nbins, double *r2_out, double *r4_out, bool *bad)
{
    const double dx = cur[0] - org[0], dy = cur[1] - org[1], dz = cur[2] - org[2];
    const double r2 = (dx * dx + dy * dy) + dz * dz, r4 = r2 * r2;
    if (!(std::fabs(r4) < 0x1p40)) {
        *bad = true;
        *r2_out = *r4_out = 0.0;
        return nbins;
    }
    *r2_out = r2;
    *r4_out = r4;
    const double q = std::sqrt(r2) / dr;   // the true quotient, correctly rounded, truncated
    return q < (double)nbins ? (int)q : nbins;
}

void add_words(uint64_t *row, __int128 x)
{
    const uint64_t add[3] = {(uint64_t)x, (uint64_t)(x >> 64), x < 0 ? ~0ull : 0ull};
    uint64_t sum[3] = {row[0], row[1], row[2]};
    ljmdk::add192(sum, add);
    row[0] = sum[0];
    row[1] = sum[1];
    row[2] = sum[2];
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

// the step kernel's stand-in: ru of particle i, axis c moves by (c + 1) (i % 7 + 1) 2^-10 per step -- exact in doubles
hipError_t launch_batch(const BatchArgs &a, int n_max, int n_blocks, hipStream_t s)
{
    g_log.push_back({'B', a.g0, n_max, n_blocks, s, a.step0, a.nsteps, 0, 0, 0, 0});
    if (a.mode != kModeSteps) return hipSuccess;
    for (int k = 0; k < n_blocks; ++k) {
        const BatchReplica &rp = a.rep[a.g0 + k];
        for (int c = 0; c < 3; ++c)
            for (int i = 0; i < rp.n; ++i)
                a.state[(size_t)(3 + c) * a.plane + rp.off + i] += a.nsteps * (c + 1) * (i % 7 + 1) * 0x1p-10;
    }
    return hipSuccess;
}

hipError_t launch_batch_fixed(const BatchFixedArgs &a, int n_max, int n_blocks, hipStream_t s)
{
    return launch_batch(a.b, n_max, n_blocks, s);
}

hipError_t launch_batch_rdf(const BatchRdfArgs &a, int n_max, int n_blocks, hipStream_t s)
{
    g_log.push_back({'R', a.g0, n_max, n_blocks, s, 0, 0, 0, 0, 0, 0});
    return hipSuccess;
}

hipError_t launch_batch_tcf(const BatchTcfArgs &a, int n_max, int n_blocks, hipStream_t s)
{
    g_log.push_back({'T', a.g0, n_max, n_blocks, s, 0, 0, 0, 0, 0, 0});
    if (g_tcf_flags >= 0) a.range[g_tcf_flags] = 1;
    return hipSuccess;
}

// the meaning of batch_vanhove_kernel, replica by replica and origin by origin
hipError_t launch_batch_vanhove(const BatchVanhoveArgs &a, int n_max, int n_blocks, hipStream_t s)
{
    g_log.push_back({'V', a.g0, n_max, n_blocks, s, 0, 0, a.n_live, a.lag_first, a.slot_first, a.store_slot});
    check(a.state && a.ring && a.hist && a.sums && a.range && a.dr && a.inv_dr && a.rep && a.plane > 0,
          "a van Hove launch has all its pointers");
    check(a.nbins >= 1 && a.nbins <= kBatchVanhoveMaxBins && a.max_lag >= 1 && a.stride >= 1 && a.slots == a.max_lag / a.stride + 1 &&
              a.n_live >= 0 && a.n_live <= a.slots && a.slot_first >= 0 && a.slot_first < a.slots && a.store_slot < a.slots &&
              (a.n_live == 0 || (a.lag_first <= a.max_lag && a.lag_first - (a.n_live - 1) * a.stride >= 1)),
          "a van Hove launch has a valid window");
    if (g_fail_vanhove > 0 && --g_fail_vanhove == 0) return hipErrorLaunchFailure;
    const int rows = a.max_lag + 1, cols = a.nbins + 1;
    for (int k = 0; k < n_blocks; ++k) {
        const BatchReplica &rp = a.rep[a.g0 + k];
        check(a.inv_dr[rp.b] == 1.0 / a.dr[rp.b], "1 / dr beside dr");
        const bool lag0 = a.n_live > 0 && a.lag_first - (a.n_live - 1) * a.stride == 1;
        for (int e = 0; e < a.n_live + (lag0 ? 1 : 0); ++e) {
            const bool zero = e == a.n_live;
            const int slot = (a.slot_first + (zero ? a.n_live - 1 : e)) % a.slots;
            const int lag = zero ? 0 : a.lag_first - e * a.stride;
            const double *const o = a.ring + (size_t)slot * 3 * a.plane + rp.off;
            __int128 s2 = 0, s4 = 0;
            for (int i = 0; i < rp.n; ++i) {
                double cur[3], org[3], r2, r4;
                bool bad = false;
                for (int c = 0; c < 3; ++c) {
                    org[c] = o[(size_t)c * a.plane + i];
                    cur[c] = zero ? org[c] : a.state[(size_t)(3 + c) * a.plane + rp.off + i];
                }
                const int bin = term(cur, org, a.dr[rp.b], a.nbins, &r2, &r4, &bad);
                if (bad) a.range[rp.b] = 1;
                ++a.hist[((size_t)rp.b * rows + lag) * cols + bin];
                s2 += Q(r2);
                s4 += Q(r4);
            }
            add_words(a.sums + (((size_t)rp.b * 2 + 0) * rows + lag) * 3, s2);
            add_words(a.sums + (((size_t)rp.b * 2 + 1) * rows + lag) * 3, s4);
        }
        if (a.store_slot >= 0)
            for (int c = 0; c < 3; ++c)
                for (int i = 0; i < rp.n; ++i)
                    a.ring[((size_t)a.store_slot * 3 + c) * a.plane + rp.off + i] = a.state[(size_t)(3 + c) * a.plane + rp.off + i];
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
const double kRmax[kB] = {0.25, 0.5, 1.0};

ljmd_batch_t *create()
{
    ljmd_batch_t *h = nullptr;
    check(ljmd_batch_create_per_replica(&h, kB, kN, kL, kDt, kRc, LJMD_PRECISION_FP64, 0) == LJMD_OK && h, "create");
    return h;
}

// positions on a grid of 2^-4 inside the box: every later ru is a multiple of 2^-10
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

// the resident ru of every replica: [3][total]
std::vector<double> snapshot(ljmd_batch_t *h)
{
    std::vector<double> u(3 * h->total);
    check(ljmd_batch_get_state(h, nullptr, nullptr, nullptr, u.data(), u.data() + h->total, u.data() + 2 * h->total, nullptr,
                               nullptr, nullptr, nullptr, nullptr, nullptr) == LJMD_OK, "get_state");
    return u;
}

// the definition, by brute force over the stored snapshots of the trajectories
struct Brute {
    int max_lag, stride, nbins;
    std::vector<uint64_t> H;               // [B][rows][cols]
    std::vector<__int128> S;               // [B][2][rows]
    std::vector<int64_t> counts;           // [rows]
    int64_t snapshots = 0;
    Brute(int max_lag_, int stride_, int nbins_)
        : max_lag(max_lag_), stride(stride_), nbins(nbins_), H((size_t)kB * (max_lag_ + 1) * (nbins_ + 1), 0),
          S((size_t)kB * 2 * (max_lag_ + 1), 0), counts((size_t)max_lag_ + 1, 0) {}
    void add(const ljmd_batch_t *h, const std::vector<double> &cur, const std::vector<double> &org, int lag)
    {
        const size_t rows = (size_t)max_lag + 1, cols = (size_t)nbins + 1;
        for (size_t b = 0; b < h->B; ++b)
            for (int i = 0; i < h->rep[b].n; ++i) {
                const size_t k = (size_t)h->offsets[b] + i;
                const double c[3] = {cur[k], cur[h->total + k], cur[2 * h->total + k]};
                const double o[3] = {org[k], org[h->total + k], org[2 * h->total + k]};
                double r2, r4;
                bool bad = false;
                const int bin = term(c, o, kRmax[b] / nbins, nbins, &r2, &r4, &bad);
                ++H[(b * rows + lag) * cols + bin];
                S[(b * 2 + 0) * rows + lag] += Q(r2);
                S[(b * 2 + 1) * rows + lag] += Q(r4);
            }
        ++counts[lag];
    }
    void trajectory(const ljmd_batch_t *h, const std::vector<std::vector<double>> &snaps)
    {
        const int64_t n = (int64_t)snaps.size();
        for (int64_t t0 = 0; t0 < n; t0 += stride) {
            if (t0 + 1 < n) add(h, snaps[t0], snaps[t0], 0);       // lag 0 once the next snapshot has arrived
            for (int64_t s = t0 + 1; s < n && s - t0 <= max_lag; ++s) add(h, snaps[s], snaps[t0], (int)(s - t0));
        }
        snapshots += n;
    }
};

void compare(ljmd_batch_t *h, const Brute &want, const char *what)
{
    const size_t rows = (size_t)want.max_lag + 1, cols = (size_t)want.nbins + 1;
    std::vector<uint64_t> hist(kB * rows * cols, 99), hist2(hist);
    std::vector<int64_t> words(kB * 2 * rows * 3, 99), counts(rows, 99), counts2(rows, 99);
    std::vector<double> r2(kB * rows, -1.0), r4(kB * rows, -1.0);
    int64_t snaps = -1, snaps2 = -1;
    check(ljmd_batch_vanhove_read_exact(h, hist.data(), words.data(), counts.data(), &snaps) == LJMD_OK, what);
    check(ljmd_batch_vanhove_read(h, hist2.data(), r2.data(), r4.data(), counts2.data(), &snaps2) == LJMD_OK, what);
    bool ok = hist == want.H && hist2 == want.H && counts == want.counts && counts2 == want.counts && snaps == want.snapshots &&
              snaps2 == want.snapshots;
    for (size_t b = 0; b < (size_t)kB; ++b)
        for (size_t kind = 0; kind < 2; ++kind)
            for (size_t l = 0; l < rows; ++l) {
                const int64_t *w = words.data() + ((b * 2 + kind) * rows + l) * 3;
                const __int128 x = want.S[(b * 2 + kind) * rows + l];
                ok = ok && (uint64_t)w[0] == (uint64_t)x && (uint64_t)w[1] == (uint64_t)(x >> 64) && w[2] == (x < 0 ? -1 : 0);
                double q = -1.0;
                ok = ok && ljmd_tcf_from_exact(w, kN[b], counts[l], &q) == LJMD_OK && q == (kind ? r4 : r2)[b * rows + l];
                uint64_t sum = 0;
                for (size_t c = 0; c < cols; ++c) sum += hist[(b * rows + l) * cols + c];
                ok = ok && sum == (uint64_t)kN[b] * (uint64_t)counts[l];
            }
    check(ok, what);
}

// 1. the guards: codes and messages, in the header's order
void guards()
{
    const std::string cfg = "ljmd_batch_vanhove_configure: ";
    check(ljmd_batch_vanhove_configure(nullptr, -1, 0, 0, nullptr, -1) == LJMD_ERR_INVALID_ARG &&
              message_is(nullptr, cfg + "NULL handle"), "configure: NULL handle first");
    check(ljmd_batch_vanhove_accumulate(nullptr) == LJMD_ERR_INVALID_ARG && ljmd_batch_vanhove_reset(nullptr) == LJMD_ERR_INVALID_ARG &&
              ljmd_batch_vanhove_read(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == LJMD_ERR_INVALID_ARG &&
              ljmd_batch_vanhove_read_exact(nullptr, nullptr, nullptr, nullptr, nullptr) == LJMD_ERR_INVALID_ARG &&
              message_is(nullptr, "ljmd_batch_vanhove_read_exact: NULL handle"), "the other calls: NULL handle");
    ljmd_batch_t *h = create();
    if (!h) return;
    const long base = g_live;
    const double nan = std::nan(""), inf = INFINITY;
    const double bad1[kB] = {0.5, 0.0, nan}, bad2[kB] = {0.5, 0.5, inf}, bad0[kB] = {-1.0, 0.5, 0.5}, tiny[kB] = {0.5, 1e-310, 0.5};
    struct Case { int max_lag, stride, nbins; const double *rmax; int every; std::string msg; };
    const Case cases[] = {
        {-1, 0, 0, nullptr, -1, cfg + "max_lag = -1 outside 1..4096 (0 switches the van Hove function off)"},
        {4097, 0, 0, nullptr, -1, cfg + "max_lag = 4097 outside 1..4096 (0 switches the van Hove function off)"},
        {0, 0, 0, nullptr, -1, cfg + "every must be >= 0"},
        {3, 0, 0, nullptr, 0, cfg + "origin_stride must be >= 1"},
        {512, 1, 0, nullptr, 0, cfg + "max_lag / origin_stride + 1 = 513 exceeds LJMD_BATCH_VANHOVE_MAX_ORIGINS (512)"},
        {3, 1, 0, nullptr, 0, cfg + "nbins = 0 outside 1..1024"},
        {3, 1, 1025, nullptr, 0, cfg + "nbins = 1025 outside 1..1024"},
        {3, 1, 8, nullptr, 0, cfg + "rmax is NULL"},
        {3, 1, 8, bad1, 0, cfg + "replica 1: rmax must be finite and > 0"},
        {3, 1, 8, bad2, 0, cfg + "replica 2: rmax must be finite and > 0"},
        {3, 1, 8, bad0, 0, cfg + "replica 0: rmax must be finite and > 0"},
        {3, 1, 1024, tiny, 0, cfg + "replica 1: rmax / nbins is not a normal number"},
    };
    for (const Case &c : cases)
        check(ljmd_batch_vanhove_configure(h, c.max_lag, c.stride, c.nbins, c.rmax, c.every) == LJMD_ERR_INVALID_ARG &&
                  message_is(h, c.msg), c.msg.c_str());
    check(g_live == base && h->vanhove.max_lag == 0 && !h->vanhove.release && !h->vanhove.acc.enqueue,
          "the refused calls allocate nothing and leave the handle's entries empty");
    const char *first = "call ljmd_batch_vanhove_configure first";
    check(ljmd_batch_vanhove_accumulate(h) == LJMD_ERR_STATE && message_is(h, std::string("ljmd_batch_vanhove_accumulate: ") + first),
          "accumulate before configure");
    check(ljmd_batch_vanhove_read(h, nullptr, nullptr, nullptr, nullptr, nullptr) == LJMD_ERR_STATE &&
              ljmd_batch_vanhove_read_exact(h, nullptr, nullptr, nullptr, nullptr) == LJMD_ERR_STATE &&
              ljmd_batch_vanhove_reset(h) == LJMD_ERR_STATE && message_is(h, std::string("ljmd_batch_vanhove_reset: ") + first),
          "read, read_exact, reset before configure");

    // the entry guard: van Hove is asked behind the heat flux and before the state
    const unsigned all = kNeedVanhove | kNeedState | kNeedSound;
    check(enter(h, "who", all | kNeedHeatflux) == LJMD_ERR_STATE && message_has(h, "call ljmd_batch_heatflux_configure first"),
          "the heat flux is asked before it");
    check(enter(h, "who", all) == LJMD_ERR_STATE && message_is(h, std::string("who: ") + first), "then van Hove");

    // configure: five buffers, their byte counts in size_t, in this order
    g_allocs.clear();
    check(ljmd_batch_vanhove_configure(h, 7, 2, 16, kRmax, 0) == LJMD_OK && g_live == base + 5, "configure allocates five buffers");
    const size_t total = 5 + 130 + 8;
    const std::vector<size_t> want = {(size_t)kB * 8 * 17 * 8, (size_t)kB * 2 * 8 * 3 * 8, (size_t)kB * 4, (size_t)2 * kB * 8,
                                      (size_t)4 * 3 * total * 8};
    check(g_allocs == want, "H, sums, range words, dr / inv_dr, the ring of 4 slots x 3 planes");
    check(h->vanhove.slots == 4 && h->vanhove.nbins == 16 && h->vanhove.d_dr[1] == 0.5 / 16 && h->vanhove.d_dr[kB + 2] == 16.0,
          "slots, and dr_b = rmax[b] / nbins with its reciprocal");
    check(enter(h, "who", all) == LJMD_ERR_STATE && message_has(h, "no state has been set"), "then the state");
    check(ljmd_batch_vanhove_configure(h, 3, 1, 0, kRmax, 0) == LJMD_ERR_INVALID_ARG && h->vanhove.max_lag == 7 && g_live == base + 5,
          "a failed guard keeps the earlier configuration");
    check(ljmd_batch_vanhove_accumulate(h) == LJMD_ERR_STATE && message_has(h, "no state has been set"), "accumulate before a state");
    check(set_grid_state(h, 0) == LJMD_OK, "set_state");
    h->poisoned = true;
    check(ljmd_batch_vanhove_accumulate(h) == LJMD_ERR_STATE && message_has(h, "poisoned"), "accumulate on a poisoned handle");
    int64_t snaps = -1;
    check(ljmd_batch_vanhove_read(h, nullptr, nullptr, nullptr, nullptr, &snaps) == LJMD_OK && snaps == 0, "a poisoned handle may still be read");
    h->poisoned = false;
    g_log.clear();
    check(ljmd_batch_vanhove_accumulate(h) == LJMD_OK && only('V').size() == 2 && g_log.size() == 2, "accumulate needs no accelerations");

    // a failed allocation: everything released, the feature off, the message naming buffer and bytes
    g_fail_alloc_of = (size_t)6 * 3 * total * 8;
    check(ljmd_batch_vanhove_configure(h, 5, 1, 16, kRmax, 0) == LJMD_ERR_ALLOC &&
              message_is(h, cfg + "cannot allocate 20592 bytes of the origin ring (6 slots)") && g_live == base &&
              h->vanhove.max_lag == 0 && !h->vanhove.release, "a failed allocation: LJMD_ERR_ALLOC with the feature off");
    g_fail_alloc_of = 0;
    check(ljmd_batch_vanhove_accumulate(h) == LJMD_ERR_STATE, "off after it");
    check(ljmd_batch_vanhove_configure(h, 5, 1, 16, kRmax, 0) == LJMD_OK && g_live == base + 5, "configure again");
    check(ljmd_batch_vanhove_configure(h, 0, -5, -5, nullptr, 0) == LJMD_OK && g_live == base && !h->vanhove.release,
          "configure(0) frees it, whatever the other arguments");
    check(ljmd_batch_vanhove_configure(h, 5, 1, 16, kRmax, 0) == LJMD_OK, "once more: destroyed while configured");
    ljmd_batch_destroy(h);
    check(g_live == 0, "destroy frees everything");
}

// 2. accumulate against the brute-force loop: several shapes, ring wrap, a new trajectory, reset
void against_brute_force()
{
    const int shapes[][3] = {{8, 1, 128}, {5, 3, 7}, {7, 2, 1}, {3, 1, 1024}};
    for (const auto &sh : shapes) {
        ljmd_batch_t *h = create();
        if (!h) return;
        check(ljmd_batch_vanhove_configure(h, sh[0], sh[1], sh[2], kRmax, 0) == LJMD_OK, "configure");
        Brute want(sh[0], sh[1], sh[2]);
        for (int traj = 0; traj < 2; ++traj) {
            check(set_grid_state(h, traj) == LJMD_OK && ljmd_batch_compute_forces(h, nullptr, nullptr, nullptr) == LJMD_OK, "state");
            check(h->vanhove.s == 0, "set_state restarts the numbering");
            std::vector<std::vector<double>> snaps;
            const int n_snap = traj == 0 ? 3 * (sh[0] / sh[1] + 1) + 2 : 4;       // several ring revolutions, then a short one
            for (int s = 0; s < n_snap; ++s) {
                if (s) check(steps(h, 1 + s % 3) == LJMD_OK, "steps");
                snaps.push_back(snapshot(h));
                g_log.clear();
                check(ljmd_batch_vanhove_accumulate(h) == LJMD_OK, "accumulate");
                const ljmdh::TcfWindow w = ljmdh::tcf_window(s, sh[0], sh[1], sh[0] / sh[1] + 1);
                const bool none = w.n_live == 0 && w.store_slot < 0;
                bool ok = g_log.size() == (none ? 0u : 2u);
                for (size_t g = 0; g < g_log.size(); ++g)
                    ok = ok && g_log[g].kind == 'V' && g_log[g].stream == h->stream && g_log[g].g0 == (int)h->groups[g].first &&
                         g_log[g].n_blocks == (int)h->groups[g].count && g_log[g].n_max == h->groups[g].n_max &&
                         g_log[g].n_live == w.n_live && g_log[g].lag_first == w.lag_first && g_log[g].slot_first == w.slot_first &&
                         g_log[g].store_slot == w.store_slot;
                check(ok, "one launch per group on the handle's stream with the window of tcf_window(s)");
            }
            want.trajectory(h, snaps);
            compare(h, want, traj == 0 ? "the first trajectory equals the brute-force loop" : "both trajectories average together");
        }
        check(ljmd_batch_vanhove_reset(h) == LJMD_OK && h->vanhove.s == 0, "reset");
        compare(h, Brute(sh[0], sh[1], sh[2]), "reset zeroes histogram, sums, counts and numbering");
        ljmd_batch_destroy(h);
        check(g_live == 0, "destroy frees everything");
    }
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
    check(steps(h, 12) == LJMD_OK, "steps without van Hove");
    const std::vector<Launch> before = g_log;
    check(only('V').empty() && !only('R').empty() && !only('T').empty(), "its transcript");
    auto restart = [&] {
        return ljmd_batch_tcf_reset(h) == LJMD_OK && set_grid_state(h, 0) == LJMD_OK &&
               ljmd_batch_compute_forces(h, nullptr, nullptr, nullptr) == LJMD_OK;
    };
    check(ljmd_batch_vanhove_configure(h, 4, 1, 16, kRmax, 0) == LJMD_OK && restart(), "configure with every == 0");
    g_log.clear();
    check(steps(h, 12) == LJMD_OK && g_log == before, "every == 0: the same launches");
    check(ljmd_batch_vanhove_configure(h, 0, 0, 0, nullptr, 0) == LJMD_OK && restart(), "configure(0)");
    g_log.clear();
    check(steps(h, 12) == LJMD_OK && g_log == before, "switched off: the same launches");

    // every = 3 beside 4 (g(r)) and 2 (MSD / VACF): a launch ends at the multiples of any of them
    check(ljmd_batch_vanhove_configure(h, 4, 1, 16, kRmax, 3) == LJMD_OK && restart(), "configure(every = 3)");
    std::vector<std::vector<double>> snaps;
    snaps.push_back(snapshot(h));
    check(ljmd_batch_vanhove_accumulate(h) == LJMD_OK, "snapshot 0 by hand");
    g_log.clear();
    check(steps(h, 8) == LJMD_ERR_INVALID_ARG && g_log.empty() &&
              message_is(h, "ljmd_batch_steps: nsteps 8 is not a multiple of the van Hove interval 3 (ljmd_batch_vanhove_configure: every)"),
          "nsteps % every != 0 is refused before anything launches");
    check(steps(h, 9) == LJMD_ERR_INVALID_ARG && message_has(h, "g(r) interval 4"), "g(r) is asked before it");
    check(steps(h, 12) == LJMD_OK && h->vanhove.s == 5 && h->vanhove.snapshots == 5, "steps(12): four snapshots, counted once each");
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
            if (mine[i].kind != 'V') continue;
            // the last launch of its step: behind the step launch that ends at 3 (k + 1) and the other accumulators'
            size_t prev = i - 1;
            while (prev > 0 && (mine[prev].kind == 'R' || mine[prev].kind == 'T')) --prev;
            const ljmdh::TcfWindow w = ljmdh::tcf_window(1 + k, 4, 1, 5);
            ok = ok && i > 0 && mine[prev].kind == 'B' && mine[prev].step0 + mine[prev].nsteps == 3 * (k + 1) &&
                 (i + 1 == mine.size() || mine[i + 1].kind == 'B') && mine[i].n_blocks == (int)g.count && mine[i].n_max == g.n_max &&
                 mine[i].n_live == w.n_live && mine[i].lag_first == w.lag_first && mine[i].slot_first == w.slot_first &&
                 mine[i].store_slot == w.store_slot;
            ++k;
        }
        check(ok && k == 4 && ends == 8, "a group's van Hove launches end its steps 3, 6, 9, 12 on its own stream; cuts at 2 3 4 6 8 9 10 12");
    }
    // the snapshots inside steps are ru0 + 3 k steps of the stand-in: the manual sequence gives the same integers
    {
        ljmd_batch_t *m = create();
        if (m) {
            check(set_grid_state(m, 0) == LJMD_OK && ljmd_batch_compute_forces(m, nullptr, nullptr, nullptr) == LJMD_OK &&
                      ljmd_batch_vanhove_configure(m, 4, 1, 16, kRmax, 0) == LJMD_OK && ljmd_batch_vanhove_accumulate(m) == LJMD_OK, "the manual route");
            for (int k = 0; k < 4; ++k) {
                check(steps(m, 3) == LJMD_OK, "steps(3)");
                snaps.push_back(snapshot(m));
                check(ljmd_batch_vanhove_accumulate(m) == LJMD_OK, "accumulate");
            }
            ljmd_batch_destroy(m);
        }
        Brute want(4, 1, 16);
        want.trajectory(h, snaps);
        compare(h, want, "every = 3 inside steps equals steps(3) + accumulate, and the brute-force loop");
    }

    // the sticky range word: the arrays are filled, the lowest replica is named, no poison, reset clears it
    {
        std::vector<double> u = snapshot(h);
        u[(size_t)h->offsets[2] + 1] += 1.0e6;
        u[(size_t)h->offsets[1] + 7] += 1.0e6;
        check(ljmd_batch_set_unwrapped(h, u.data(), u.data() + h->total, u.data() + 2 * h->total) == LJMD_OK &&
                  ljmd_batch_vanhove_accumulate(h) == LJMD_OK, "two replicas out of range");
        const size_t rows = 5, cols = 17;
        std::vector<uint64_t> hist(kB * rows * cols, 99);
        std::vector<int64_t> words(kB * 2 * rows * 3, 99), counts(rows, 99);
        std::vector<double> r2(kB * rows, -1.0);
        int64_t n_snap = -1;
        check(ljmd_batch_vanhove_read_exact(h, hist.data(), words.data(), counts.data(), &n_snap) == LJMD_ERR_RANGE &&
                  message_has(h, "ljmd_batch_vanhove_read_exact: replica 1: a van Hove displacement") &&
                  message_has(h, "until ljmd_batch_vanhove_reset") && !h->poisoned, "LJMD_ERR_RANGE names the lowest replica; no poison");
        check(n_snap == 6 && counts[1] == 5 && hist[(1 * rows + 1) * cols + 16] >= 1 && hist[(2 * rows + 4) * cols + 16] >= 1 &&
                  words[0] != 99, "... with the arrays filled and the particles in the overflow column");
        check(ljmd_batch_vanhove_read(h, nullptr, r2.data(), nullptr, nullptr, nullptr) == LJMD_ERR_RANGE && r2[1] >= 0.0,
              "read likewise");
        check(steps(h, 12) == LJMD_OK, "stepping goes on");
        check(ljmd_batch_vanhove_read(h, nullptr, nullptr, nullptr, nullptr, nullptr) == LJMD_ERR_RANGE, "sticky");
        check(ljmd_batch_vanhove_reset(h) == LJMD_OK && ljmd_batch_vanhove_read(h, nullptr, nullptr, nullptr, nullptr, &n_snap) == LJMD_OK &&
                  n_snap == 0, "reset clears it");
    }

    // an injected launch failure: poison, then recovery through set_state
    check(restart() && steps(h, 12) == LJMD_OK && h->vanhove.snapshots == 4, "four snapshots");
    g_fail_vanhove = 2;
    g_log.clear();
    check(steps(h, 12) == LJMD_ERR_HIP && message_has(h, "ljmd_batch_steps: van Hove launch failed") && message_has(h, "poisoned") &&
              h->poisoned && only('V').size() == 2, "an injected launch failure poisons the handle");
    check(h->vanhove.snapshots == 4 && h->vanhove.s == 4, "... and leaves counts and numbering alone");
    check(steps(h, 12) == LJMD_ERR_STATE && ljmd_batch_vanhove_accumulate(h) == LJMD_ERR_STATE, "poisoned until set_state");
    check(ljmd_batch_vanhove_reset(h) == LJMD_OK && restart() && !h->poisoned && steps(h, 12) == LJMD_OK && h->vanhove.snapshots == 4 &&
              h->vanhove.max_lag == 4 && h->vanhove.every == 3, "set_state recovers and keeps the configuration");
    ljmd_batch_destroy(h);
    check(g_live == 0, "destroy frees everything (three accumulators on)");
}

// 4. MSD / VACF, the other observable of the same ring rules: a set range word fails its reads BEFORE anything is written
// to the caller's arrays, counts or n_snapshots -- where the van Hove reads above fill everything and then fail
void tcf_read_on_range()
{
    const int32_t n[kB] = {8, 8, 8};
    ljmd_batch_t *h = nullptr;
    check(ljmd_batch_create_per_replica(&h, kB, n, kL, kDt, kRc, LJMD_PRECISION_FP64, 0) == LJMD_OK && h, "create (n = 8)");
    if (!h) return;
    check(set_grid_state(h, 0) == LJMD_OK && ljmd_batch_tcf_configure(h, 2, 1, 0) == LJMD_OK, "state, MSD / VACF configured");
    g_tcf_flags = 1;
    g_log.clear();
    check(ljmd_batch_tcf_accumulate(h) == LJMD_OK && only('T').size() == 1, "one snapshot, whose launch sets replica 1's range word");
    g_tcf_flags = -1;
    const size_t rows = 3;
    const double sd = -7.0;
    const int64_t si = 99;
    std::vector<double> msd(kB * rows, sd), vacf(kB * rows, sd);
    std::vector<int64_t> words(kB * 2 * rows * 3, si), counts(rows, si);
    int64_t n_snap = si;
    auto untouched = [&] {
        bool ok = n_snap == si;
        for (double x : msd) ok = ok && x == sd;
        for (double x : vacf) ok = ok && x == sd;
        for (int64_t x : words) ok = ok && x == si;
        for (int64_t x : counts) ok = ok && x == si;
        return ok;
    };
    check(ljmd_batch_tcf_read(h, msd.data(), vacf.data(), counts.data(), &n_snap) == LJMD_ERR_RANGE &&
              message_has(h, "ljmd_batch_tcf_read: replica 1: an MSD or VACF term") && message_has(h, "until ljmd_batch_tcf_reset") &&
              !h->poisoned, "ljmd_batch_tcf_read: LJMD_ERR_RANGE names replica 1; no poison");
    check(untouched(), "... with msd, vacf, counts and n_snapshots untouched");
    check(ljmd_batch_tcf_read_exact(h, words.data(), counts.data(), &n_snap) == LJMD_ERR_RANGE &&
              message_has(h, "ljmd_batch_tcf_read_exact: replica 1: an MSD or VACF term") && !h->poisoned,
          "ljmd_batch_tcf_read_exact: LJMD_ERR_RANGE names replica 1; no poison");
    check(untouched(), "... with words, counts and n_snapshots untouched");
    check(ljmd_batch_tcf_reset(h) == LJMD_OK && ljmd_batch_tcf_read(h, msd.data(), vacf.data(), counts.data(), &n_snap) == LJMD_OK &&
              n_snap == 0 && counts[0] == 0 && msd[0] == 0.0 && vacf[kB * rows - 1] == 0.0 &&
              ljmd_batch_tcf_read_exact(h, words.data(), counts.data(), &n_snap) == LJMD_OK && words[0] == 0,
          "after ljmd_batch_tcf_reset the reads succeed and fill their arrays");
    ljmd_batch_destroy(h);
    check(g_live == 0, "destroy frees everything (MSD / VACF alone)");
}

}  // namespace

int main()
{
    setenv("FAKEHIP_DEVICES", "1", 1);
    unsetenv("LJMD_BATCH_GROUP_STREAMS");
    guards();
    against_brute_force();
    inside_steps();
    tcf_read_on_range();
    if (g_failures == 0) std::printf("batch_vanhove_host: ok\n");
    return g_failures == 0 ? 0 : 1;
}
