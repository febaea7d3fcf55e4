// tcf_host.cpp -- TEST INFRASTRUCTURE: the host core of the engine's resident MSD / VACF (csrc/ljmd_tcf.cpp, namespace
// ljmdt) without a GPU and without the engine.  Linked from the core, ljmd_common.cpp, the fake HIP runtime
// (tests/fakehip: hipMalloc is calloc) and its own definitions of the three launchers, which check what they are given
// and then carry out the kernels' meaning on the host in plain loops with __int128.  The program checks itself -- a
// brute-force sum over stored snapshots against the words the core returns (several (max_lag, stride) pairs, a slot
// permutation that changes between snapshots, ring wrap, a new trajectory), every guard with its return code and
// message, the arguments of every launch, and the byte counts of configure for n up to 2^23 -- prints one line per check
// that fails and "tcf_host: ok" when none did.  tests/test_tcf_host.py runs it under ASan and UBSan.  (The fake hipMalloc
// cannot fail, so the LJMD_ERR_ALLOC branch of configure is not reached here.)
#include "ljmd.h"
#include "ljmd_internal.h"
#include "ljmd_resident.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <random>
#include <string>
#include <vector>

using namespace ljmdt;

namespace {

int g_failures = 0;
int g_gathers = 0, g_terms = 0, g_folds = 0;
int g_fail_terms = 0;                      // 1: the next terms launch returns hipErrorLaunchFailure
const TcfState *g_st = nullptr;            // the state under test: the launchers check their pointers against it
TcfGatherArgs g_gather{};
TcfTermsArgs g_last{};

void check(bool ok, const char *what)
{
    if (ok) return;
    ++g_failures;
    std::printf("FAILED: %s\n", what);
}

bool has(const std::string &err, const char *text) { return err.find(text) != std::string::npos; }

// Q(t) = RNE(t 2^64) as an integer; out of range -> 0 and the flag
__int128 q_of(double t, bool &bad)
{
    if (!(std::fabs(t) < 0x1p40)) {
        bad = true;
        return 0;
    }
    const double v = std::nearbyint(t * 0x1p64);
    const double h = std::trunc(v * 0x1p-52);
    return (__int128)(long long)h * ((__int128)1 << 52) + (__int128)(long long)(v - h * 0x1p52);
}

double msd_term(const double *c, const double *o, size_t np, size_t i)
{
    const double dx = c[0 * np + i] - o[0 * np + i], dy = c[1 * np + i] - o[1 * np + i], dz = c[2 * np + i] - o[2 * np + i];
    return (dx * dx + dy * dy) + dz * dz;
}

double vacf_term(const double *c, const double *o, size_t np, size_t i)
{
    return (c[3 * np + i] * o[3 * np + i] + c[4 * np + i] * o[4 * np + i]) + c[5 * np + i] * o[5 * np + i];
}

bool window_ok(int nblk, int slots, int ents, int stride, int n_live, int lag_first, int chunk, int slices)
{
    return nblk == g_st->sz.nblk && slots == g_st->sz.slots && ents == slots + 1 && stride == g_st->stride && n_live >= 1 &&
           n_live <= slots && lag_first <= g_st->max_lag && lag_first - (n_live - 1) * stride >= 1 && chunk >= 1 &&
           chunk <= kTcfMaxChunk && (long long)slices * chunk >= n_live && (long long)(slices - 1) * chunk < n_live;
}

}  // namespace

namespace ljmdt {

hipError_t launch_tcf_gather(const TcfGatherArgs &a, hipStream_t)
{
    ++g_gathers;
    g_gather = a;
    check(a.ru && a.v && a.perm && a.cur == g_st->d_cur && a.n == g_st->n && a.P >= a.n && a.n_pad == g_st->sz.n_pad,
          "gather launch: arguments");
    if (a.store) {
        const size_t off = (size_t)(a.store - g_st->d_ring), slot = off / (6 * a.n_pad);
        check(off % (6 * a.n_pad) == 0 && slot < (size_t)g_st->sz.slots, "gather launch: the store slot lies in the ring");
    }
    for (int s = 0; s < a.P; ++s) {
        const int id = a.perm[s];
        if (id < 0 || id >= a.n) continue;
        for (int c = 0; c < 6; ++c) {
            const double x = c < 3 ? a.ru[(size_t)c * a.P + s] : a.v[(size_t)(c - 3) * a.P + s];
            a.cur[(size_t)c * a.n_pad + id] = x;
            if (a.store) a.store[(size_t)c * a.n_pad + id] = x;
        }
    }
    return hipSuccess;
}

hipError_t launch_tcf_terms(const TcfTermsArgs &a, hipStream_t)
{
    ++g_terms;
    if (g_fail_terms > 0 && --g_fail_terms == 0) return hipErrorLaunchFailure;
    g_last = a;
    check(a.cur == g_st->d_cur && a.ring == g_st->d_ring && a.part == g_st->d_part && a.flag == g_st->d_flag &&
              a.n_pad == g_st->sz.n_pad && a.n_pad == (size_t)a.nblk * kTcfBlock, "terms launch: buffers");
    check(window_ok(a.nblk, a.slots, a.ents, a.stride, a.n_live, a.lag_first, a.chunk, a.slices) && a.slot_first >= 0 &&
              a.slot_first < a.slots, "terms launch: window and slices");
    check((long long)a.nblk * a.slices >= std::min<long long>(kTcfTargetWorkgroups, (long long)a.nblk * a.n_live) / 2,
          "terms launch: the grid is filled where the live origins allow it");
    if (g_gather.store) {       // the slot stored in this snapshot is not among the live ones
        const int store = (int)((size_t)(g_gather.store - a.ring) / (6 * a.n_pad));
        for (int e = 0; e < a.n_live; ++e) check((a.slot_first + e) % a.slots != store, "terms launch: the stored slot is not live");
    }
    const size_t np = a.n_pad;
    for (int blk = 0; blk < a.nblk; ++blk)
        for (int slice = 0; slice < a.slices; ++slice) {
            const int e0 = slice * a.chunk, e1 = std::min(a.n_live, e0 + a.chunk);
            const bool lag0 = e1 == a.n_live && a.lag_first - (a.n_live - 1) * a.stride == 1;
            bool bad = false;
            for (int e = e0; e < e1 + (lag0 ? 1 : 0); ++e) {
                const bool zero = e == a.n_live;
                const int slot = (a.slot_first + (zero ? a.n_live - 1 : e)) % a.slots;
                const double *o = a.ring + (size_t)slot * 6 * np, *c = zero ? o : a.cur;
                __int128 sum[2] = {0, 0};
                for (size_t i = (size_t)blk * kTcfBlock; i < (size_t)(blk + 1) * kTcfBlock; ++i) {
                    sum[0] += q_of(msd_term(c, o, np, i), bad);
                    sum[1] += q_of(vacf_term(c, o, np, i), bad);
                }
                for (int kind = 0; kind < 2; ++kind) {
                    unsigned long long *w = a.part + (((size_t)blk * a.ents + e) * 2 + kind) * 2;
                    w[0] = (unsigned long long)sum[kind];
                    w[1] = (unsigned long long)(sum[kind] >> 64);
                }
            }
            a.flag[(size_t)blk * a.slots + slice] = bad ? 1 : 0;
        }
    return hipSuccess;
}

hipError_t launch_tcf_fold(const TcfFoldArgs &a, hipStream_t)
{
    ++g_folds;
    check(a.part == g_st->d_part && a.flag == g_st->d_flag && a.sums == g_st->d_sums && a.range == g_st->d_range &&
              a.max_lag == g_st->max_lag, "fold launch: buffers");
    check(window_ok(a.nblk, a.slots, a.ents, a.stride, a.n_live, a.lag_first, a.chunk, a.slices) &&
              a.n_live == g_last.n_live && a.lag_first == g_last.lag_first && a.chunk == g_last.chunk &&
              a.slices == g_last.slices, "fold launch: the window of the terms launch");
    const bool lag0 = a.lag_first - (a.n_live - 1) * a.stride == 1;
    for (int e = 0; e < a.n_live + (lag0 ? 1 : 0); ++e)
        for (int kind = 0; kind < 2; ++kind) {
            const int lag = e < a.n_live ? a.lag_first - e * a.stride : 0;
            uint64_t tot[3] = {0, 0, 0};
            for (int b = 0; b < a.nblk; ++b) {
                const unsigned long long *p = a.part + (((size_t)b * a.ents + e) * 2 + kind) * 2;
                const uint64_t add[3] = {p[0], p[1], (long long)p[1] < 0 ? ~0ull : 0ull};
                ljmdk::add192(tot, add);
            }
            uint64_t *row = a.sums + ((size_t)kind * (a.max_lag + 1) + lag) * 3;
            uint64_t sum[3] = {row[0], row[1], row[2]};
            ljmdk::add192(sum, tot);
            row[0] = sum[0]; row[1] = sum[1]; row[2] = sum[2];
        }
    for (int b = 0; b < a.nblk; ++b)
        for (int y = 0; y < a.slices; ++y)
            if (a.flag[(size_t)b * a.slots + y]) *a.range = 1;
    return hipSuccess;
}

}  // namespace ljmdt

namespace {

// an "engine": n particles in P slots, slot s holding particle perm[s]
struct Sys {
    int n, P;
    std::vector<double> ru, v;      // [3][P] slot order
    std::vector<int> perm;
    std::vector<double> id_ru, id_v;   // [3][n] particle-id order: the truth
    std::mt19937_64 rng{12345};

    explicit Sys(int n_) : n(n_), P((n_ + 255) / 256 * 256), ru(3 * (size_t)P), v(3 * (size_t)P), perm(P), id_ru(3 * (size_t)n_),
                           id_v(3 * (size_t)n_)
    {
        std::iota(perm.begin(), perm.end(), 0);
    }
    ResidentView view() const
    {
        ResidentView w;
        w.n = n; w.P = P; w.G = 1;
        w.ru = ru.data(); w.v = v.data(); w.perm = perm.data();
        return w;
    }
    // new values for every particle, and a new slot order
    void advance(bool shuffle)
    {
        std::uniform_real_distribution<double> u(-3.0, 3.0);
        for (auto &x : id_ru) x += u(rng);
        for (auto &x : id_v) x = u(rng);
        if (shuffle) std::shuffle(perm.begin(), perm.end(), rng);      // padding ids (>= n) land anywhere
        for (int s = 0; s < P; ++s)
            for (int c = 0; c < 3; ++c) {
                const int id = perm[s];
                ru[(size_t)c * P + s] = id < n ? id_ru[(size_t)c * n + id] : 777.0;   // junk on the padding slots
                v[(size_t)c * P + s] = id < n ? id_v[(size_t)c * n + id] : -777.0;
            }
    }
};

struct Brute {
    int max_lag, stride, n;
    std::vector<__int128> S;        // [2][max_lag + 1]
    std::vector<int64_t> counts;
    std::vector<std::vector<double>> snaps;   // of the current trajectory: [6][n]
    Brute(int ml, int st, int n_) : max_lag(ml), stride(st), n(n_), S(2 * (size_t)(ml + 1), 0), counts((size_t)ml + 1, 0) {}
    void push(const Sys &y)
    {
        std::vector<double> z(6 * (size_t)n);
        std::copy(y.id_ru.begin(), y.id_ru.end(), z.begin());
        std::copy(y.id_v.begin(), y.id_v.end(), z.begin() + 3 * (size_t)n);
        snaps.push_back(z);
    }
    // closes the trajectory: every (origin, later snapshot) pair, and lag 0 of every origin that has a successor
    void close()
    {
        const int m = (int)snaps.size();
        bool bad = false;
        for (int t0 = 0; t0 < m; t0 += stride)
            for (int s = t0; s < m && s - t0 <= max_lag; ++s) {
                if (s == t0 && t0 + 1 >= m) continue;
                for (int i = 0; i < n; ++i) {
                    S[(size_t)(s - t0)] += q_of(msd_term(snaps[s].data(), snaps[t0].data(), n, i), bad);
                    S[(size_t)(max_lag + 1 + s - t0)] += q_of(vacf_term(snaps[s].data(), snaps[t0].data(), n, i), bad);
                }
                ++counts[(size_t)(s - t0)];
            }
        check(!bad, "brute force: terms in range");
        snaps.clear();
    }
};

void compare(TcfState &st, const Sys &y, const Brute &b, const char *what)
{
    std::string err;
    const size_t rows = (size_t)b.max_lag + 1;
    std::vector<uint64_t> words(2 * rows * 3);
    std::vector<int64_t> counts(rows);
    std::vector<double> msd(rows), vacf(rows);
    int64_t snaps = -1;
    check(tcf_fetch(&st, &err, "caller", y.view(), words.data(), counts.data(), &snaps) == LJMD_OK, what);
    check(tcf_read(&st, &err, "caller", y.view(), msd.data(), vacf.data(), nullptr, nullptr) == LJMD_OK, what);
    bool same = counts == b.counts;
    for (size_t k = 0; k < 2 * rows; ++k) {
        const __int128 x = b.S[k];
        same = same && words[3 * k] == (uint64_t)x && words[3 * k + 1] == (uint64_t)(x >> 64) &&
               words[3 * k + 2] == (x < 0 ? ~0ull : 0ull);
        const uint64_t w3[3] = {words[3 * k], words[3 * k + 1], words[3 * k + 2]};
        const int64_t c = counts[k % rows];
        const double want = c ? ljmdk::fixed_to_double(w3) / ((double)y.n * (double)c) : 0.0;
        same = same && (k < rows ? msd[k] : vacf[k - rows]) == want;
    }
    if (!same) std::printf("case %s: max_lag %d stride %d n %d\n", what, b.max_lag, b.stride, y.n);
    check(same, "the core's words, counts and quotients equal the brute-force sums");
    check(b.S[1] != 0 && b.S[rows] != 0, "the brute-force sums are not trivially zero");
}

void run_case(int n, int max_lag, int stride, int n_snap, int second_trajectory)
{
    Sys y(n);
    TcfState st;
    g_st = &st;
    std::string err;
    Brute b(max_lag, stride, n);
    check(tcf_configure(&st, &err, "caller", y.view(), max_lag, stride) == LJMD_OK, "configure");
    for (int s = 0; s < n_snap; ++s) {
        y.advance(true);
        check(tcf_accumulate(&st, &err, "caller", y.view()) == LJMD_OK, "accumulate");
        b.push(y);
    }
    b.close();
    compare(st, y, b, "one trajectory");
    if (second_trajectory > 0) {
        tcf_new_trajectory(&st);
        for (int s = 0; s < second_trajectory; ++s) {
            y.advance(s % 2 == 0);
            check(tcf_accumulate(&st, &err, "caller", y.view()) == LJMD_OK, "accumulate");
            b.push(y);
        }
        b.close();
        compare(st, y, b, "two trajectories");
        int64_t snaps = 0;
        check(tcf_fetch(&st, &err, "caller", y.view(), nullptr, nullptr, &snaps) == LJMD_OK && snaps == n_snap + second_trajectory,
              "the snapshot count runs over both trajectories");
    }
    tcf_release(&st, nullptr);
}

void brute_force()
{
    run_case(1500, 4, 1, 10, 0);        // two particle blocks
    run_case(1500, 5, 2, 10, 7);        // n_live reaches the slot count (3), and a second trajectory
    run_case(300, 3, 5, 12, 0);         // stride > max_lag: one slot
    run_case(300, 6, 6, 14, 5);
    run_case(70, 40, 1, 100, 0);        // ring wrap, many slices
    run_case(5, 511, 1, 520, 0);        // 512 slots, every slot reused, slices of one origin
    run_case(2, 1, 1, 3, 2);
}

void guards_and_sequences()
{
    Sys y(1000);
    y.advance(true);
    const ResidentView v = y.view();
    TcfState st;
    g_st = &st;
    std::string err;
    const char *who = "caller";
    int64_t snaps = -1, counts[8];
    uint64_t words[2 * 8 * 3];
    double ms = -1.0, msd[8];
    int32_t live = -1;
    const int g0 = g_gathers, t0 = g_terms, f0 = g_folds;

    // before configure
    check(tcf_accumulate(&st, &err, who, v) == LJMD_ERR_STATE && has(err, "caller: MSD / VACF is not configured"), "accumulate before configure");
    check(tcf_fetch(&st, &err, who, v, words, counts, &snaps) == LJMD_ERR_STATE && has(err, "not configured"), "read_exact before configure");
    check(tcf_read(&st, &err, who, v, msd, nullptr, counts, &snaps) == LJMD_ERR_STATE && has(err, "not configured"), "read before configure");
    check(tcf_reset(&st, &err, who, v) == LJMD_ERR_STATE && has(err, "not configured"), "reset before configure");
    check(tcf_profile_read(&st, &err, who, v, &ms, &live) == LJMD_ERR_STATE, "profile_read before configure");
    check(g_gathers == g0 && g_terms == t0, "nothing launched before configure");

    // guards of configure, each leaving what was there
    check(tcf_configure(&st, &err, who, v, -1, 1) == LJMD_ERR_INVALID_ARG && has(err, "caller: max_lag = -1 outside 1..4096"), "max_lag < 0");
    check(tcf_configure(&st, &err, who, v, 4097, 16) == LJMD_ERR_INVALID_ARG && has(err, "max_lag = 4097"), "max_lag too large");
    check(tcf_configure(&st, &err, who, v, 3, 0) == LJMD_ERR_INVALID_ARG && has(err, "caller: origin_stride must be >= 1"), "stride 0");
    check(tcf_configure(&st, &err, who, v, 512, 1) == LJMD_ERR_INVALID_ARG && has(err, "= 513 exceeds LJMD_TCF_MAX_ORIGINS (512)"), "too many origins");
    check(tcf_configure(&st, &err, who, v, 1024, 2) == LJMD_ERR_INVALID_ARG && has(err, "exceeds LJMD_TCF_MAX_ORIGINS"), "too many origins, stride 2");
    ResidentView rank = v;
    rank.G = 2;
    check(tcf_configure(&st, &err, who, rank, 4, 1) == LJMD_ERR_INVALID_ARG && has(err, "caller: n_ranks = 2") &&
              has(err, "needs a one-rank engine"), "a rank engine is refused");
    ResidentView multi = v;
    multi.multi = true; multi.G = 2; multi.ru = multi.v = nullptr; multi.perm = nullptr;
    check(tcf_configure(&st, &err, who, multi, 4, 1) == LJMD_ERR_INVALID_ARG && has(err, "n_ranks") && has(err, "multi-device"),
          "a multi-device handle is refused");
    check(tcf_configure(&st, &err, who, multi, 0, 0) == LJMD_OK, "max_lag = 0 is accepted anywhere");
    check(st.max_lag == 0 && !st.d_ring && !st.d_cur && !st.d_sums && !st.d_part && !st.d_flag && !st.d_range,
          "refused configure allocates nothing");
    check(tcf_accumulate(&st, &err, who, rank) == LJMD_ERR_STATE && has(err, "not configured"), "rank engine: not configured");

    check(tcf_configure(&st, &err, who, v, 7, 2) == LJMD_OK && st.max_lag == 7 && st.stride == 2 && st.sz.slots == 4 &&
              st.sz.n_pad == 1024 && st.sz.nblk == 1 && st.d_ring && st.d_cur && st.d_sums, "configure");
    check(tcf_configure(&st, &err, who, v, 5000, 1) == LJMD_ERR_INVALID_ARG && st.max_lag == 7 && st.stride == 2,
          "a refused reconfigure keeps the configuration");
    check(tcf_configure(&st, &err, who, v, 7, -3) == LJMD_ERR_INVALID_ARG && st.max_lag == 7, "a refused stride keeps it too");
    check(tcf_fetch(&st, &err, who, v, words, counts, &snaps) == LJMD_OK && snaps == 0 && words[0] == 0 && counts[0] == 0 && counts[7] == 0,
          "zeroed by configure");
    check(tcf_profile_read(&st, &err, who, v, &ms, &live) == LJMD_OK && ms == 0.0 && live == 0, "profile before the first accumulate");

    // the sequence of launches: the first snapshot meets no origin
    check(tcf_accumulate(&st, &err, who, v) == LJMD_OK && g_gathers == g0 + 1 && g_terms == t0 && g_folds == f0,
          "snapshot 0: the gather alone");
    check(g_gather.store == st.d_ring && g_gather.ru == v.ru && g_gather.v == v.v && g_gather.perm == v.perm, "snapshot 0 is stored in slot 0");
    check(tcf_profile_read(&st, &err, who, v, &ms, &live) == LJMD_OK && live == 0, "profile: no live origin yet");
    check(tcf_accumulate(&st, &err, who, v) == LJMD_OK && g_terms == t0 + 1 && g_folds == f0 + 1 && g_gather.store == nullptr &&
              g_last.n_live == 1 && g_last.lag_first == 1 && g_last.slot_first == 0, "snapshot 1: origin 0 at lag 1, not stored");
    check(tcf_accumulate(&st, &err, who, v) == LJMD_OK && g_gather.store == st.d_ring + 6 * st.sz.n_pad && g_last.n_live == 1 &&
              g_last.lag_first == 2, "snapshot 2: stored in slot 1");
    check(tcf_fetch(&st, &err, who, v, nullptr, counts, &snaps) == LJMD_OK && snaps == 3 && counts[0] == 1 && counts[1] == 1 &&
              counts[2] == 1 && counts[3] == 0, "counts after three snapshots");
    check(tcf_fetch(&st, &err, who, v, nullptr, nullptr, nullptr) == LJMD_OK && tcf_read(&st, &err, who, v, nullptr, nullptr, nullptr, nullptr) == LJMD_OK,
          "reads with NULL pointers");
    check(tcf_profile_read(&st, &err, who, v, &ms, &live) == LJMD_OK && live == 1, "profile: the most recent accumulate");
    check(tcf_profile_read(&st, &err, who, v, nullptr, nullptr) == LJMD_OK, "profile with NULL pointers");

    // a failed launch: reported, not counted
    g_fail_terms = 1;
    check(tcf_accumulate(&st, &err, who, v) == LJMD_ERR_HIP && has(err, "caller: MSD / VACF launch failed"), "failed launch");
    check(tcf_fetch(&st, &err, who, v, nullptr, counts, &snaps) == LJMD_OK && snaps == 3 && counts[1] == 1, "failed launch adds no snapshot");

    // an engine of another size is refused
    Sys other(900);
    check(tcf_accumulate(&st, &err, who, other.view()) == LJMD_ERR_STATE, "a view of another n");

    // range: sticky until reset, read clears nothing
    Sys far = y;
    far.id_ru[3] += 0x1p21;
    far.advance(false);
    check(tcf_accumulate(&st, &err, who, far.view()) == LJMD_OK, "accumulate with a term out of range");
    check(tcf_fetch(&st, &err, who, v, words, counts, &snaps) == LJMD_ERR_RANGE && has(err, "caller: an MSD or VACF term") &&
              has(err, "ljmd_tcf_reset"), "read_exact: range");
    check(tcf_read(&st, &err, who, v, msd, nullptr, nullptr, nullptr) == LJMD_ERR_RANGE, "read: range");
    check(tcf_accumulate(&st, &err, who, v) == LJMD_OK && tcf_fetch(&st, &err, who, v, nullptr, nullptr, nullptr) == LJMD_ERR_RANGE,
          "the range word is sticky");
    check(tcf_reset(&st, &err, who, v) == LJMD_OK, "reset");
    check(tcf_fetch(&st, &err, who, v, words, counts, &snaps) == LJMD_OK && snaps == 0 && counts[0] == 0 && counts[1] == 0 &&
              std::all_of(words, words + 48, [](uint64_t w) { return w == 0; }), "reset zeroes");
    check(tcf_accumulate(&st, &err, who, v) == LJMD_OK && g_gather.store == st.d_ring, "reset restarts the numbering");

    // a new trajectory: origins dropped, counts kept
    check(tcf_accumulate(&st, &err, who, v) == LJMD_OK, "second snapshot");
    tcf_new_trajectory(&st);
    const int t1 = g_terms;
    check(tcf_accumulate(&st, &err, who, v) == LJMD_OK && g_terms == t1 && g_gather.store == st.d_ring, "new trajectory: no origin is live");
    check(tcf_fetch(&st, &err, who, v, nullptr, counts, &snaps) == LJMD_OK && snaps == 3 && counts[1] == 1, "new trajectory keeps the counts");

    // reconfigure zeroes, off frees
    check(tcf_configure(&st, &err, who, v, 3, 1) == LJMD_OK && st.max_lag == 3 && st.snapshots == 0 && st.s == 0 && st.sz.slots == 4, "reconfigure");
    check(tcf_configure(&st, &err, who, v, 0, 0) == LJMD_OK && st.max_lag == 0 && !st.d_ring && !st.d_cur && !st.d_sums && !st.timer.ev0 && !st.timer.ev1,
          "off frees");
    check(tcf_accumulate(&st, &err, who, v) == LJMD_ERR_STATE && tcf_reset(&st, &err, who, v) == LJMD_ERR_STATE, "off: as before configure");
    check(tcf_configure(&st, &err, who, v, 2, 1) == LJMD_OK, "configure again");
    tcf_release(&st, nullptr);                               // what ljmd_destroy does on a configured handle
    check(st.max_lag == 0 && !st.d_ring, "release");
    tcf_release(&st, nullptr);                               // and on one that is not
}

// byte counts in size_t, and a grid for every number of live origins
void sizes_and_slices()
{
    const int ns[] = {1, 2, 1023, 1024, 1025, 4096, 65536, 262144, 1048576, (1 << 23) - 1, 1 << 23};
    const int cfg[][2] = {{1, 1}, {5, 2}, {511, 1}, {4096, 9}, {4088, 8}, {4096, 4096}};
    for (int n : ns)
        for (auto &c : cfg) {
            const TcfSizes z = tcf_sizes(n, c[0], c[1]);
            const unsigned __int128 np = ((unsigned __int128)n + 1023) / 1024 * 1024, slots = (unsigned)(c[0] / c[1] + 1);
            const bool ok = z.slots == (int)slots && z.slots <= kTcfMaxOrigins && z.ents == z.slots + 1 && z.n_pad == (size_t)np &&
                            z.n_pad >= (size_t)n && z.n_pad - (size_t)n < 1024 && (size_t)z.nblk * 1024 == z.n_pad &&
                            (unsigned __int128)z.cur_bytes == 48 * np && (unsigned __int128)z.ring_bytes == slots * 48 * np &&
                            (unsigned __int128)z.part_bytes == (np / 1024) * (slots + 1) * 32 &&
                            (unsigned __int128)z.flag_bytes == (np / 1024) * slots * 4 && z.sums_bytes == 2 * ((size_t)c[0] + 1) * 24;
            if (!ok) std::printf("sizes of n = %d, max_lag %d, stride %d\n", n, c[0], c[1]);
            check(ok, "byte counts of configure");
        }
    check(tcf_sizes(262144, 511, 1).ring_bytes == 6442450944ull, "the ring of n = 262 144 with 512 slots: 6.4e9 bytes");
    check(tcf_sizes(1 << 23, 511, 1).ring_bytes == 206158430208ull, "the ring of n = 2^23 does not wrap a 32-bit product");
    const int blks[] = {1, 2, 3, 4, 7, 64, 256, 1000, 1024, 1025, 8192};
    for (int nblk : blks)
        for (int n_live = 1; n_live <= kTcfMaxOrigins; ++n_live) {
            const TcfSlices p = tcf_plan_slices(nblk, n_live);
            const bool ok = p.chunk >= 1 && p.chunk <= kTcfMaxChunk && p.slices >= 1 && p.slices <= n_live &&
                            (long long)p.slices * p.chunk >= n_live && (long long)(p.slices - 1) * p.chunk < n_live &&
                            (long long)nblk * p.slices >= std::min<long long>(kTcfTargetWorkgroups, (long long)nblk * n_live) / 2;
            if (!ok) std::printf("slices of nblk = %d, n_live = %d: chunk %d slices %d\n", nblk, n_live, p.chunk, p.slices);
            check(ok, "slice plan");
        }
    // the premise of test_gpu_tcf_resident.py::test_slices_of_more_than_one_origin (n = 33000: nblk = 33, max_lag = 37)
    check(tcf_plan_slices(33, 32).chunk == 1, "nblk 33: 32 live origins still have slices of one origin");
    const int want_slices[] = {17, 17, 18, 18, 19};
    for (int l = 33; l <= 37; ++l) {
        const TcfSlices p = tcf_plan_slices(33, l);
        if (p.chunk != 2 || p.slices != want_slices[l - 33]) std::printf("nblk 33, n_live %d: chunk %d slices %d\n", l, p.chunk, p.slices);
        check(p.chunk == 2 && p.slices == want_slices[l - 33], "nblk 33: from 33 live origins on, slices of two origins");
    }
}

}  // namespace

int main()
{
    setenv("FAKEHIP_DEVICES", "1", 1);
    guards_and_sequences();
    brute_force();
    sizes_and_slices();
    check(g_gathers > 600 && g_terms > 600 && g_folds == g_terms - 1, "the launchers ran");
    if (g_failures == 0) std::printf("tcf_host: ok\n");
    return g_failures == 0 ? 0 : 1;
}
