// vanhove_host.cpp -- TEST INFRASTRUCTURE: the host core of the engine's resident van Hove self-correlation
// (csrc/ljmd_vanhove.cpp, namespace ljmdv) without a GPU and without the engine.  Linked from the core, ljmd_common.cpp,
// the fake HIP runtime (tests/fakehip: hipMalloc is calloc) and its own definitions of the three launchers, which check
// what they are given and then carry out the kernels' meaning on the host in plain loops with __int128.  The program
// checks itself -- a brute-force loop over stored snapshots against the counts and words the core returns (several
// (max_lag, stride, nbins), a slot permutation that changes between snapshots, ring wrap, a new trajectory, chunk
// overrides 1, 2, 3 and >= n_live), every guard with its return code and message, the arguments of every launch, the
// byte counts of configure for n up to 2^23, the refusal of rank and multi views -- prints one line per check that fails
// and "vanhove_host: ok" when none did.  tests/test_vanhove_host.py runs it under ASan and UBSan.  (The fake hipMalloc
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

using namespace ljmdv;

namespace {

int g_failures = 0;
int g_gathers = 0, g_terms = 0, g_folds = 0;
int g_fail_terms = 0;                      // 1: the next terms launch returns hipErrorLaunchFailure
const VanHoveState *g_st = nullptr;        // the state under test: the launchers check their pointers against it
VhGatherArgs g_gather{};
VhTermsArgs g_last{};

void check(bool ok, const char *what)
{
    if (ok) return;
    ++g_failures;
    std::printf("FAILED: %s\n", what);
}

bool has(const std::string &err, const char *text) { return err.find(text) != std::string::npos; }

// Q(t) = RNE(t 2^64) as an integer, |t| < 2^40
__int128 q_of(double t)
{
    const double v = std::nearbyint(t * 0x1p64);
    const double h = std::trunc(v * 0x1p-52);
    return (__int128)(long long)h * ((__int128)1 << 52) + (__int128)(long long)(v - h * 0x1p52);
}

// one particle's term of the definition: bin (nbins = overflow), Q(r2), Q(r4); out of range -> overflow, 0, 0 and the flag
struct Term {
    int bin;
    __int128 q2, q4;
};
Term term_of(const double *c, const double *o, size_t np, size_t i, int nbins, double dr, bool &bad)
{
    const double dx = c[0 * np + i] - o[0 * np + i], dy = c[1 * np + i] - o[1 * np + i], dz = c[2 * np + i] - o[2 * np + i];
    const double r2 = (dx * dx + dy * dy) + dz * dz, r4 = r2 * r2;
    if (!(std::fabs(r4) < 0x1p40)) {
        bad = true;
        return {nbins, 0, 0};
    }
    const double q = std::sqrt(r2) / dr;                       // the true quotient
    return {q < (double)nbins ? (int)q : nbins, q_of(r2), q_of(r4)};
}

bool window_ok(int nblk, int slots, int ents, int stride, int n_live, int lag_first, int chunk, int slices)
{
    return nblk == g_st->sz.nblk && slots == g_st->sz.slots && ents == slots + 1 && stride == g_st->stride && n_live >= 1 &&
           n_live <= slots && lag_first <= g_st->max_lag && lag_first - (n_live - 1) * stride >= 1 && chunk >= 1 &&
           chunk <= kVhMaxChunk && (long long)slices * chunk >= n_live && (long long)(slices - 1) * chunk < n_live;
}

}  // namespace

namespace ljmdv {

hipError_t launch_vanhove_gather(const VhGatherArgs &a, hipStream_t)
{
    ++g_gathers;
    g_gather = a;
    check(a.ru && a.perm && a.cur == g_st->d_cur && a.n == g_st->n && a.P >= a.n && a.n_pad == g_st->sz.n_pad,
          "gather launch: arguments");
    if (a.store) {
        const size_t off = (size_t)(a.store - g_st->d_ring), slot = off / (3 * a.n_pad);
        check(off % (3 * a.n_pad) == 0 && slot < (size_t)g_st->sz.slots, "gather launch: the store slot lies in the ring");
    }
    for (int s = 0; s < a.P; ++s) {
        const int id = a.perm[s];
        if (id < 0 || id >= a.n) continue;
        for (int c = 0; c < 3; ++c) {
            const double x = a.ru[(size_t)c * a.P + s];
            a.cur[(size_t)c * a.n_pad + id] = x;
            if (a.store) a.store[(size_t)c * a.n_pad + id] = x;
        }
    }
    return hipSuccess;
}

hipError_t launch_vanhove_terms(const VhTermsArgs &a, hipStream_t)
{
    ++g_terms;
    if (g_fail_terms > 0 && --g_fail_terms == 0) return hipErrorLaunchFailure;
    g_last = a;
    check(a.cur == g_st->d_cur && a.ring == g_st->d_ring && a.hist == g_st->d_hist && a.part == g_st->d_part &&
              a.flag == g_st->d_flag && a.n_pad == g_st->sz.n_pad && a.n_pad == (size_t)a.nblk * kVhBlock, "terms launch: buffers");
    check(a.n == g_st->n && a.nbins == g_st->nbins && a.max_lag == g_st->max_lag && a.dr == g_st->rmax / g_st->nbins &&
              a.inv_dr == 1.0 / a.dr, "terms launch: bins");
    check(window_ok(a.nblk, a.slots, a.ents, a.stride, a.n_live, a.lag_first, a.chunk, a.slices) && a.slot_first >= 0 &&
              a.slot_first < a.slots, "terms launch: window and slices");
    if (g_gather.store) {       // the slot stored in this snapshot is not among the live ones
        const int store = (int)((size_t)(g_gather.store - a.ring) / (3 * a.n_pad));
        for (int e = 0; e < a.n_live; ++e) check((a.slot_first + e) % a.slots != store, "terms launch: the stored slot is not live");
    }
    const size_t np = a.n_pad, cols = (size_t)a.nbins + 1;
    for (int blk = 0; blk < a.nblk; ++blk)
        for (int slice = 0; slice < a.slices; ++slice) {
            const int e0 = slice * a.chunk, e1 = std::min(a.n_live, e0 + a.chunk);
            const bool lag0 = e1 == a.n_live && a.lag_first - (a.n_live - 1) * a.stride == 1;
            bool bad = false;
            for (int e = e0; e < e1 + (lag0 ? 1 : 0); ++e) {
                const bool zero = e == a.n_live;
                const int slot = (a.slot_first + (zero ? a.n_live - 1 : e)) % a.slots;
                const int lag = zero ? 0 : a.lag_first - e * a.stride;
                const double *o = a.ring + (size_t)slot * 3 * np, *c = zero ? o : a.cur;
                __int128 sum[2] = {0, 0};
                for (size_t i = (size_t)blk * kVhBlock; i < (size_t)(blk + 1) * kVhBlock; ++i) {
                    const Term t = term_of(c, o, np, i, a.nbins, a.dr, bad);
                    sum[0] += t.q2;
                    sum[1] += t.q4;
                    if (i < (size_t)a.n) ++a.hist[(size_t)lag * cols + t.bin];       // the padding ids are not counted
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

hipError_t launch_vanhove_fold(const VhFoldArgs &a, hipStream_t)
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

}  // namespace ljmdv

namespace {

// an "engine": n particles in P slots, slot s holding particle perm[s]
struct Sys {
    int n, P;
    std::vector<double> ru;         // [3][P] slot order
    std::vector<int> perm;
    std::vector<double> id_ru;      // [3][n] particle-id order: the truth
    std::mt19937_64 rng{12345};
    std::optional<int> chunk;

    explicit Sys(int n_) : n(n_), P((n_ + 255) / 256 * 256), ru(3 * (size_t)P), perm(P), id_ru(3 * (size_t)n_)
    {
        std::iota(perm.begin(), perm.end(), 0);
    }
    ResidentView view() const
    {
        ResidentView w;
        w.n = n; w.P = P; w.G = 1;
        w.ru = ru.data(); w.perm = perm.data();
        w.vanhove_chunk = chunk;
        return w;
    }
    // new values for every particle, and a new slot order
    void advance(bool shuffle)
    {
        std::uniform_real_distribution<double> u(-0.5, 0.5);
        for (auto &x : id_ru) x += u(rng);
        if (shuffle) std::shuffle(perm.begin(), perm.end(), rng);      // padding ids (>= n) land anywhere
        for (int s = 0; s < P; ++s)
            for (int c = 0; c < 3; ++c) {
                const int id = perm[s];
                ru[(size_t)c * P + s] = id < n ? id_ru[(size_t)c * n + id] : 777.0;   // junk on the padding slots
            }
    }
};

struct Brute {
    int max_lag, stride, n, nbins;
    double dr;
    std::vector<__int128> S;        // [2][max_lag + 1]
    std::vector<uint64_t> H;        // [max_lag + 1][nbins + 1]
    std::vector<int64_t> counts;
    std::vector<std::vector<double>> snaps;   // of the current trajectory: [3][n]
    Brute(int ml, int st, int n_, int nb, double rmax)
        : max_lag(ml), stride(st), n(n_), nbins(nb), dr(rmax / nb), S(2 * (size_t)(ml + 1), 0),
          H((size_t)(ml + 1) * (nb + 1), 0), counts((size_t)ml + 1, 0) {}
    void push(const Sys &y) { snaps.push_back(y.id_ru); }
    // closes the trajectory: every (origin, later snapshot) pair, and lag 0 of every origin that has a successor
    void close()
    {
        const int m = (int)snaps.size();
        bool bad = false;
        for (int t0 = 0; t0 < m; t0 += stride)
            for (int s = t0; s < m && s - t0 <= max_lag; ++s) {
                if (s == t0 && t0 + 1 >= m) continue;
                for (int i = 0; i < n; ++i) {
                    const Term t = term_of(snaps[s].data(), snaps[t0].data(), n, i, nbins, dr, bad);
                    S[(size_t)(s - t0)] += t.q2;
                    S[(size_t)(max_lag + 1 + s - t0)] += t.q4;
                    ++H[(size_t)(s - t0) * (nbins + 1) + t.bin];
                }
                ++counts[(size_t)(s - t0)];
            }
        check(!bad, "brute force: terms in range");
        snaps.clear();
    }
};

void compare(VanHoveState &st, const Sys &y, const Brute &b, const char *what)
{
    std::string err;
    const size_t rows = (size_t)b.max_lag + 1, cols = (size_t)b.nbins + 1;
    std::vector<uint64_t> words(2 * rows * 3), hist(rows * cols), hist2(rows * cols);
    std::vector<int64_t> counts(rows);
    std::vector<double> r2(rows), r4(rows);
    int64_t snaps = -1;
    check(vanhove_fetch(&st, &err, "caller", y.view(), hist.data(), words.data(), counts.data(), &snaps) == LJMD_OK, what);
    check(vanhove_read(&st, &err, "caller", y.view(), hist2.data(), r2.data(), r4.data(), nullptr, nullptr) == LJMD_OK, what);
    bool same = counts == b.counts && hist == b.H && hist2 == b.H;
    for (size_t l = 0; l < rows; ++l) {
        uint64_t sum = 0;
        for (size_t c = 0; c < cols; ++c) sum += hist[l * cols + c];
        same = same && sum == (uint64_t)y.n * (uint64_t)counts[l];
    }
    for (size_t k = 0; k < 2 * rows; ++k) {
        const __int128 x = b.S[k];
        same = same && words[3 * k] == (uint64_t)x && words[3 * k + 1] == (uint64_t)(x >> 64) &&
               words[3 * k + 2] == (x < 0 ? ~0ull : 0ull);
        const uint64_t w3[3] = {words[3 * k], words[3 * k + 1], words[3 * k + 2]};
        const int64_t c = counts[k % rows];
        const double want = c ? ljmdk::fixed_to_double(w3) / ((double)y.n * (double)c) : 0.0;
        same = same && (k < rows ? r2[k] : r4[k - rows]) == want;
    }
    if (!same) std::printf("case %s: max_lag %d stride %d nbins %d n %d\n", what, b.max_lag, b.stride, b.nbins, y.n);
    check(same, "the core's counts, words and quotients equal the brute-force loop");
    check(b.S[1] != 0 && b.S[rows + 1] != 0, "the brute-force sums are not trivially zero");
}

void run_case(int n, int max_lag, int stride, int nbins, double rmax, int n_snap, int second_trajectory,
              std::optional<int> chunk = std::nullopt)
{
    Sys y(n);
    y.chunk = chunk;
    VanHoveState st;
    g_st = &st;
    std::string err;
    Brute b(max_lag, stride, n, nbins, rmax);
    check(vanhove_configure(&st, &err, "caller", y.view(), max_lag, stride, nbins, rmax) == LJMD_OK, "configure");
    int max_chunk = 0, max_live = 0;
    for (int s = 0; s < n_snap; ++s) {
        y.advance(true);
        const int t0 = g_terms;
        check(vanhove_accumulate(&st, &err, "caller", y.view()) == LJMD_OK, "accumulate");
        b.push(y);
        if (g_terms > t0) {
            max_chunk = std::max(max_chunk, g_last.chunk);
            max_live = std::max(max_live, g_last.n_live);
            if (chunk) check(g_last.chunk == std::max(1, std::min(*chunk, std::min(g_last.n_live, kVhMaxChunk))), "the chunk override, clamped");
        }
    }
    if (chunk && *chunk > 1 && max_live > 1) check(max_chunk > 1, "a slice of more than one origin was launched");
    b.close();
    compare(st, y, b, "one trajectory");
    if (second_trajectory > 0) {
        vanhove_new_trajectory(&st);
        for (int s = 0; s < second_trajectory; ++s) {
            y.advance(s % 2 == 0);
            check(vanhove_accumulate(&st, &err, "caller", y.view()) == LJMD_OK, "accumulate");
            b.push(y);
        }
        b.close();
        compare(st, y, b, "two trajectories");
        int64_t snaps = 0;
        check(vanhove_fetch(&st, &err, "caller", y.view(), nullptr, nullptr, nullptr, &snaps) == LJMD_OK &&
                  snaps == n_snap + second_trajectory, "the snapshot count runs over both trajectories");
    }
    vanhove_release(&st, nullptr);
}

void brute_force()
{
    run_case(1500, 4, 1, 64, 1.0, 10, 0);           // two particle blocks; the longest lags overflow
    run_case(1500, 5, 2, 65, 1.5, 10, 7);           // n_live reaches the slot count (3), and a second trajectory
    run_case(300, 3, 5, 1, 0.7, 12, 0);             // stride > max_lag: one slot; one bin and the overflow column
    run_case(300, 6, 6, 4096, 2.0, 14, 5);
    run_case(70, 40, 1, 33, 4.0, 100, 0);           // ring wrap, many slices
    run_case(5, 511, 1, 16, 12.0, 520, 0);          // 512 slots, every slot reused, slices of one origin
    run_case(2, 1, 1, 8, 0.5, 3, 2);
    for (int chunk : {1, 2, 3, 8, 1000})            // chunk overrides: 1, 2, 3 (a shorter last slice) and >= n_live
        run_case(1100, 8, 1, 40, 2.0, 13, 4, chunk);
    run_case(70, 140, 1, 20, 6.0, 150, 0, 1000);    // more live origins than kVhMaxChunk: the override is clamped to 128
}

void guards_and_sequences()
{
    Sys y(1000);
    y.advance(true);
    const ResidentView v = y.view();
    VanHoveState st;
    g_st = &st;
    std::string err;
    const char *who = "caller";
    int64_t snaps = -1, counts[8];
    uint64_t words[2 * 8 * 3], hist[8 * 11];
    double ms = -1.0, r2[8];
    int32_t live = -1;
    const int g0 = g_gathers, t0 = g_terms, f0 = g_folds;

    // before configure
    check(vanhove_accumulate(&st, &err, who, v) == LJMD_ERR_STATE && has(err, "caller: the van Hove function is not configured"), "accumulate before configure");
    check(vanhove_fetch(&st, &err, who, v, hist, words, counts, &snaps) == LJMD_ERR_STATE && has(err, "not configured"), "read_exact before configure");
    check(vanhove_read(&st, &err, who, v, hist, r2, nullptr, counts, &snaps) == LJMD_ERR_STATE && has(err, "not configured"), "read before configure");
    check(vanhove_reset(&st, &err, who, v) == LJMD_ERR_STATE && has(err, "not configured"), "reset before configure");
    check(vanhove_profile_read(&st, &err, who, v, &ms, &live) == LJMD_ERR_STATE, "profile_read before configure");
    check(g_gathers == g0 && g_terms == t0, "nothing launched before configure");

    // guards of configure in their order, each leaving what was there
    check(vanhove_configure(&st, &err, who, v, -1, 0, 0, 0.0) == LJMD_ERR_INVALID_ARG && has(err, "caller: max_lag = -1 outside 1..4096"), "max_lag < 0 comes first");
    check(vanhove_configure(&st, &err, who, v, 4097, 16, 10, 1.0) == LJMD_ERR_INVALID_ARG && has(err, "max_lag = 4097"), "max_lag too large");
    check(vanhove_configure(&st, &err, who, v, 3, 0, 0, 0.0) == LJMD_ERR_INVALID_ARG && has(err, "caller: origin_stride must be >= 1"), "stride 0 before nbins");
    check(vanhove_configure(&st, &err, who, v, 512, 1, 0, 0.0) == LJMD_ERR_INVALID_ARG && has(err, "= 513 exceeds LJMD_VANHOVE_MAX_ORIGINS (512)"), "too many origins before nbins");
    check(vanhove_configure(&st, &err, who, v, 1024, 2, 10, 1.0) == LJMD_ERR_INVALID_ARG && has(err, "exceeds LJMD_VANHOVE_MAX_ORIGINS"), "too many origins, stride 2");
    check(vanhove_configure(&st, &err, who, v, 4, 1, 0, -1.0) == LJMD_ERR_INVALID_ARG && has(err, "caller: nbins = 0 outside 1..4096"), "nbins 0 before rmax");
    check(vanhove_configure(&st, &err, who, v, 4, 1, 4097, 1.0) == LJMD_ERR_INVALID_ARG && has(err, "nbins = 4097"), "nbins too large");
    for (double bad : {0.0, -1.0, (double)INFINITY, (double)NAN, 4e-324})
        check(vanhove_configure(&st, &err, who, v, 4, 1, 10, bad) == LJMD_ERR_INVALID_ARG && has(err, "caller: rmax must be finite and > 0"), "rmax");
    ResidentView rank = v;
    rank.G = 2;
    check(vanhove_configure(&st, &err, who, rank, 4, 1, 10, -1.0) == LJMD_ERR_INVALID_ARG && has(err, "rmax"), "rmax before the rank check");
    check(vanhove_configure(&st, &err, who, rank, 4, 1, 10, 1.0) == LJMD_ERR_INVALID_ARG && has(err, "caller: n_ranks = 2") &&
              has(err, "needs a one-rank engine"), "a rank engine is refused");
    ResidentView multi = v;
    multi.multi = true; multi.G = 2; multi.ru = nullptr; multi.perm = nullptr;
    check(vanhove_configure(&st, &err, who, multi, 4, 1, 10, 1.0) == LJMD_ERR_INVALID_ARG && has(err, "n_ranks") && has(err, "multi-device"),
          "a multi-device handle is refused");
    ResidentView big = v;
    big.n = (1 << 23) + 1; big.P = big.n;
    check(vanhove_configure(&st, &err, who, big, 4, 1, 10, 1.0) == LJMD_ERR_INVALID_ARG && has(err, "caller: n = 8388609 outside 1..8388608"), "n too large");
    check(vanhove_configure(&st, &err, who, multi, 0, 0, 0, 0.0) == LJMD_OK, "max_lag = 0 is accepted anywhere");
    check(st.max_lag == 0 && !st.d_ring && !st.d_cur && !st.d_sums && !st.d_hist && !st.d_part && !st.d_flag && !st.d_range,
          "refused configure allocates nothing");
    for (const ResidentView *w : {&rank, &multi}) {
        check(vanhove_accumulate(&st, &err, who, *w) == LJMD_ERR_STATE && has(err, "not configured"), "rank / multi: accumulate not configured");
        check(vanhove_fetch(&st, &err, who, *w, nullptr, nullptr, nullptr, nullptr) == LJMD_ERR_STATE, "rank / multi: read_exact");
        check(vanhove_read(&st, &err, who, *w, nullptr, nullptr, nullptr, nullptr, nullptr) == LJMD_ERR_STATE, "rank / multi: read");
        check(vanhove_reset(&st, &err, who, *w) == LJMD_ERR_STATE && vanhove_profile_read(&st, &err, who, *w, nullptr, nullptr) == LJMD_ERR_STATE,
              "rank / multi: reset and profile_read");
    }

    check(vanhove_configure(&st, &err, who, v, 7, 2, 10, 2.0) == LJMD_OK && st.max_lag == 7 && st.stride == 2 && st.nbins == 10 &&
              st.rmax == 2.0 && st.dr == 0.2 && st.inv_dr == 1.0 / 0.2 && st.sz.slots == 4 && st.sz.n_pad == 1024 && st.sz.nblk == 1 &&
              st.d_ring && st.d_cur && st.d_sums && st.d_hist, "configure");
    check(vanhove_configure(&st, &err, who, v, 5000, 1, 10, 2.0) == LJMD_ERR_INVALID_ARG && st.max_lag == 7 && st.stride == 2,
          "a refused reconfigure keeps the configuration");
    check(vanhove_configure(&st, &err, who, v, 7, -3, 10, 2.0) == LJMD_ERR_INVALID_ARG && st.max_lag == 7, "a refused stride keeps it too");
    check(vanhove_configure(&st, &err, who, v, 7, 2, 10, 0.0) == LJMD_ERR_INVALID_ARG && st.nbins == 10 && st.rmax == 2.0, "a refused rmax keeps it too");
    check(vanhove_configure(&st, &err, who, rank, 7, 2, 10, 2.0) == LJMD_ERR_INVALID_ARG && st.max_lag == 7, "a refused view keeps it too");
    check(vanhove_fetch(&st, &err, who, v, hist, words, counts, &snaps) == LJMD_OK && snaps == 0 && words[0] == 0 && counts[0] == 0 &&
              counts[7] == 0 && hist[0] == 0 && hist[87] == 0, "zeroed by configure");
    check(vanhove_profile_read(&st, &err, who, v, &ms, &live) == LJMD_OK && ms == 0.0 && live == 0, "profile before the first accumulate");

    // the sequence of launches: the first snapshot meets no origin
    check(vanhove_accumulate(&st, &err, who, v) == LJMD_OK && g_gathers == g0 + 1 && g_terms == t0 && g_folds == f0,
          "snapshot 0: the gather alone");
    check(g_gather.store == st.d_ring && g_gather.ru == v.ru && g_gather.perm == v.perm && g_gather.P == v.P, "snapshot 0 is stored in slot 0");
    check(vanhove_profile_read(&st, &err, who, v, &ms, &live) == LJMD_OK && live == 0, "profile: no live origin yet");
    check(vanhove_accumulate(&st, &err, who, v) == LJMD_OK && g_terms == t0 + 1 && g_folds == f0 + 1 && g_gather.store == nullptr &&
              g_last.n_live == 1 && g_last.lag_first == 1 && g_last.slot_first == 0 && g_last.chunk == 1 && g_last.slices == 1,
          "snapshot 1: origin 0 at lag 1, not stored");
    check(vanhove_accumulate(&st, &err, who, v) == LJMD_OK && g_gather.store == st.d_ring + 3 * st.sz.n_pad && g_last.n_live == 1 &&
              g_last.lag_first == 2, "snapshot 2: stored in slot 1");
    check(vanhove_fetch(&st, &err, who, v, hist, nullptr, counts, &snaps) == LJMD_OK && snaps == 3 && counts[0] == 1 && counts[1] == 1 &&
              counts[2] == 1 && counts[3] == 0 && hist[0] == 1000 && hist[11] == 1000 && hist[22] == 1000 && hist[33] == 0,
          "counts after three snapshots of one state: everybody in bin 0");
    check(vanhove_fetch(&st, &err, who, v, nullptr, nullptr, nullptr, nullptr) == LJMD_OK &&
              vanhove_read(&st, &err, who, v, nullptr, nullptr, nullptr, nullptr, nullptr) == LJMD_OK, "reads with NULL pointers");
    check(vanhove_profile_read(&st, &err, who, v, &ms, &live) == LJMD_OK && live == 1, "profile: the most recent accumulate");
    check(vanhove_profile_read(&st, &err, who, v, nullptr, nullptr) == LJMD_OK, "profile with NULL pointers");

    // a failed launch: reported, not counted
    g_fail_terms = 1;
    check(vanhove_accumulate(&st, &err, who, v) == LJMD_ERR_HIP && has(err, "caller: van Hove launch failed"), "failed launch");
    check(vanhove_fetch(&st, &err, who, v, nullptr, nullptr, counts, &snaps) == LJMD_OK && snaps == 3 && counts[1] == 1, "failed launch adds no snapshot");

    // an engine of another size is refused
    Sys other(900);
    check(vanhove_accumulate(&st, &err, who, other.view()) == LJMD_ERR_STATE && has(err, "not the one the van Hove function was configured for"),
          "a view of another n");

    // range: r2 = 4e6 is a fine MSD term, r4 = 1.6e13 >= 2^40 is not -- overflow column, sums 0, sticky until reset
    Sys far = y;
    far.id_ru[3] += 2000.0;
    far.advance(false);
    check(vanhove_accumulate(&st, &err, who, far.view()) == LJMD_OK, "accumulate with a term out of range");
    check(vanhove_fetch(&st, &err, who, v, hist, words, counts, &snaps) == LJMD_ERR_RANGE && has(err, "caller: a van Hove displacement") &&
              has(err, "ljmd_vanhove_reset"), "read_exact: range");
    uint64_t in_overflow = 0;
    for (int l = 0; l < 8; ++l) in_overflow += hist[l * 11 + 10];
    check(in_overflow >= 1, "the particle out of range is in the overflow column");
    check(vanhove_read(&st, &err, who, v, nullptr, r2, nullptr, nullptr, nullptr) == LJMD_ERR_RANGE, "read: range");
    check(vanhove_accumulate(&st, &err, who, v) == LJMD_OK && vanhove_fetch(&st, &err, who, v, nullptr, nullptr, nullptr, nullptr) == LJMD_ERR_RANGE,
          "the range word is sticky");
    check(vanhove_reset(&st, &err, who, v) == LJMD_OK, "reset");
    check(vanhove_fetch(&st, &err, who, v, hist, words, counts, &snaps) == LJMD_OK && snaps == 0 && counts[0] == 0 && counts[1] == 0 &&
              std::all_of(words, words + 48, [](uint64_t w) { return w == 0; }) && std::all_of(hist, hist + 88, [](uint64_t w) { return w == 0; }),
          "reset zeroes");
    check(vanhove_accumulate(&st, &err, who, v) == LJMD_OK && g_gather.store == st.d_ring, "reset restarts the numbering");

    // a new trajectory: origins dropped, counts kept
    check(vanhove_accumulate(&st, &err, who, v) == LJMD_OK, "second snapshot");
    vanhove_new_trajectory(&st);
    const int t1 = g_terms;
    check(vanhove_accumulate(&st, &err, who, v) == LJMD_OK && g_terms == t1 && g_gather.store == st.d_ring, "new trajectory: no origin is live");
    check(vanhove_fetch(&st, &err, who, v, hist, nullptr, counts, &snaps) == LJMD_OK && snaps == 3 && counts[1] == 1 && hist[11] == 1000,
          "new trajectory keeps the counts");

    // reconfigure zeroes, off frees
    check(vanhove_configure(&st, &err, who, v, 3, 1, 5, 1.0) == LJMD_OK && st.max_lag == 3 && st.nbins == 5 && st.snapshots == 0 && st.s == 0 &&
              st.sz.slots == 4, "reconfigure");
    check(vanhove_configure(&st, &err, who, v, 0, 0, 0, 0.0) == LJMD_OK && st.max_lag == 0 && !st.d_ring && !st.d_cur && !st.d_sums && !st.d_hist &&
              !st.timer.ev0 && !st.timer.ev1, "off frees");
    check(vanhove_accumulate(&st, &err, who, v) == LJMD_ERR_STATE && vanhove_reset(&st, &err, who, v) == LJMD_ERR_STATE, "off: as before configure");
    check(vanhove_configure(&st, &err, who, v, 2, 1, 3, 1.0) == LJMD_OK, "configure again");
    vanhove_release(&st, nullptr);                           // what ljmd_destroy does on a configured handle
    check(st.max_lag == 0 && !st.d_ring, "release");
    vanhove_release(&st, nullptr);                           // and on one that is not
}

// byte counts in size_t, and a grid for every number of live origins, with and without the override
void sizes_and_slices()
{
    const int ns[] = {1, 2, 1023, 1024, 1025, 4096, 65536, 262144, 1048576, (1 << 23) - 1, 1 << 23};
    const int cfg[][3] = {{1, 1, 1}, {5, 2, 64}, {511, 1, 4096}, {4096, 9, 4096}, {4088, 8, 100}, {4096, 4096, 4095}};
    for (int n : ns)
        for (auto &c : cfg) {
            const VhSizes z = vanhove_sizes(n, c[0], c[1], c[2]);
            const unsigned __int128 np = ((unsigned __int128)n + 1023) / 1024 * 1024, slots = (unsigned)(c[0] / c[1] + 1);
            const bool ok = z.slots == (int)slots && z.slots <= kVhMaxOrigins && z.ents == z.slots + 1 && z.n_pad == (size_t)np &&
                            z.n_pad >= (size_t)n && z.n_pad - (size_t)n < 1024 && (size_t)z.nblk * 1024 == z.n_pad &&
                            (unsigned __int128)z.cur_bytes == 24 * np && (unsigned __int128)z.ring_bytes == slots * 24 * np &&
                            (unsigned __int128)z.part_bytes == (np / 1024) * (slots + 1) * 32 &&
                            (unsigned __int128)z.flag_bytes == (np / 1024) * slots * 4 && z.sums_bytes == 2 * ((size_t)c[0] + 1) * 24 &&
                            z.hist_bytes == ((size_t)c[0] + 1) * ((size_t)c[2] + 1) * 8;
            if (!ok) std::printf("sizes of n = %d, max_lag %d, stride %d, nbins %d\n", n, c[0], c[1], c[2]);
            check(ok, "byte counts of configure");
        }
    check(vanhove_sizes(262144, 511, 1, 4096).ring_bytes == 3221225472ull, "the ring of n = 262 144 with 512 slots: 3.2e9 bytes");
    check(vanhove_sizes(1 << 23, 511, 1, 4096).ring_bytes == 103079215104ull, "the ring of n = 2^23 does not wrap a 32-bit product");
    check(vanhove_sizes(1 << 23, 4096, 9, 4096).hist_bytes == 4097ull * 4097ull * 8ull, "the histogram of 4097 lags and 4096 bins");
    const int blks[] = {1, 2, 3, 4, 7, 64, 256, 1000, 1024, 1025, 8192};
    const int overrides[] = {0, -5, 1, 2, 3, 127, 128, 129, 512, 100000};   // 0 here = no override
    for (int nblk : blks)
        for (int n_live = 1; n_live <= kVhMaxOrigins; ++n_live)
            for (int o : overrides) {
                const VhSlices p = o == 0 ? vanhove_plan_slices(nblk, n_live) : vanhove_plan_slices(nblk, n_live, o);
                bool ok = p.chunk >= 1 && p.chunk <= kVhMaxChunk && p.chunk <= n_live && p.slices >= 1 && p.slices <= n_live &&
                          (long long)p.slices * p.chunk >= n_live && (long long)(p.slices - 1) * p.chunk < n_live;
                if (o == 0)
                    ok = ok && (long long)nblk * p.slices >= std::min<long long>(kVhTargetWorkgroups, (long long)nblk * n_live) / 2;
                else
                    ok = ok && p.chunk == std::max(1, std::min(o, std::min(n_live, kVhMaxChunk)));
                if (!ok) std::printf("slices of nblk = %d, n_live = %d, override %d: chunk %d slices %d\n", nblk, n_live, o, p.chunk, p.slices);
                check(ok, "slice plan");
            }
}

}  // namespace

int main()
{
    setenv("FAKEHIP_DEVICES", "1", 1);
    guards_and_sequences();
    brute_force();
    sizes_and_slices();
    check(g_gathers > 800 && g_terms > 800 && g_folds == g_terms - 1, "the launchers ran");
    if (g_failures == 0) std::printf("vanhove_host: ok\n");
    return g_failures == 0 ? 0 : 1;
}
