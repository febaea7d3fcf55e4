// rhok_host.cpp -- TEST INFRASTRUCTURE: the host core of the engine's resident density modes (csrc/ljmd_rhok.cpp,
// namespace ljmdc) without a GPU and without the engine.  Linked from the core, ljmd_common.cpp, the fake HIP runtime
// (tests/fakehip) and its own definitions of the two launchers, which check what they are given and carry out on the
// host what the kernels mean: units of (particle chunk, mode chunk), live slots by the permutation, rows of partials
// with their padding, flags, and the fold.  The program checks itself -- every guard with its return code and message in
// order, the refusal of rank engines and multi-device views, the sequences around configure / accumulate / read / reset,
// a full series, the entries limit, NULL outputs, release while configured, the range word, ljmd_rhok_select_modes, and
// the returned words against a brute-force sum over the particles in particle order -- prints one line per check that
// fails and "rhok_host: ok" when none did.  tests/test_rhok_host.py runs it under ASan and UBSan.
// (The fake hipMalloc cannot fail, so the LJMD_ERR_ALLOC branch of configure is not reached here.)
#include "ljmd.h"
#include "ljmd_internal.h"
#include "ljmd_resident.h"
#include "ljmd_rhok_arith.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

using namespace ljmdc;
using ljmdk::add192;
using ljmdk::from128;

namespace {

int g_failures = 0;
int g_terms = 0, g_fold = 0;
int g_fail_terms = 0;                       // 1: the next terms launch returns hipErrorLaunchFailure
RhokTermsArgs g_last{};

void check(bool ok, const char *what)
{
    if (ok) return;
    ++g_failures;
    std::printf("FAILED: %s\n", what);
}

bool has(const std::string &err, const char *text) { return err.find(text) != std::string::npos; }

// Q(t) = RNE(t 2^64) of |t| <= 2 as one integer
__int128 Q(double t)
{
    long long hi, lo;
    ljmdk::rhok_fixed_parts(t, hi, lo);
    return (__int128)hi * ((__int128)1 << 32) + lo;
}

// the definition's term of particle (x, y, z) and mode n into re / im
void add_term(const double *x, const int32_t *n, double L, __int128 &re, __int128 &im, bool &bad)
{
    double C, S;
    ljmdk::rhok_term((double)n[0], (double)n[1], (double)n[2], ljmdk::rhok_turns(x[0], L), ljmdk::rhok_turns(x[1], L),
                     ljmdk::rhok_turns(x[2], L), C, S);
    const bool oob = ljmdk::rhok_out_of_range(C, S);
    bad = bad || oob;
    re += Q(oob ? 0.0 : C);
    im += Q(oob ? 0.0 : S);
}

}  // namespace

namespace ljmdc {

// rhok_terms_kernel on the host: unit by unit, lane by lane
hipError_t launch_rhok_terms(const RhokTermsArgs &a, hipStream_t)
{
    ++g_terms;
    if (g_fail_terms > 0 && --g_fail_terms == 0) return hipErrorLaunchFailure;
    g_last = a;
    check(rhok_terms_ok(a), "terms launch: arguments");
    const RhokPlan p = rhok_plan(a.T, a.n_modes);
    check(p.mchunks == a.mchunks && p.pchunks == a.pchunks && p.tiles == a.tiles, "terms launch: the plan");
    const size_t P = (size_t)a.P;
    for (int unit = 0; unit < a.pchunks * a.mchunks; ++unit) {
        const int y = unit % a.mchunks, pc = unit / a.mchunks;
        bool any_bad = false;
        for (int lane = 0; lane < 64; ++lane) {
            const int m = y * 64 + lane;
            const bool mode_live = m < a.n_modes;
            const int32_t zero[3] = {0, 0, 0};
            const int32_t *n = mode_live ? a.modes + 3 * m : zero;
            __int128 re = 0, im = 0;
            bool bad = false;
            for (int t = pc * a.tiles; t < std::min(a.T, (pc + 1) * a.tiles); ++t)
                for (int j = 0; j < 64; ++j) {
                    const size_t s = (size_t)t * 64 + j;
                    if (a.perm[s] < 0 || a.perm[s] >= a.n) continue;
                    const double x[3] = {a.pos[s], a.pos[P + s], a.pos[2 * P + s]};
                    add_term(x, n, a.L, re, im, bad);
                }
            uint64_t q[2][3] = {};
            if (mode_live) {
                from128(q[0], re);
                from128(q[1], im);
            }
            std::memcpy(a.part + ((size_t)pc * a.mchunks * 64 + m) * kRhokRowWords, q, sizeof q);
            any_bad = any_bad || (bad && mode_live);
        }
        a.flag[(size_t)pc * a.mchunks + y] = any_bad ? 1u : 0u;
    }
    return hipSuccess;
}

hipError_t launch_rhok_fold(const RhokFoldArgs &a, hipStream_t)
{
    ++g_fold;
    check(rhok_fold_ok(a), "fold launch: arguments");
    bool bad = false;
    for (int m = 0; m < a.n_modes; ++m) {
        uint64_t q[2][3] = {};
        for (int p = 0; p < a.pchunks; ++p)
            for (int c = 0; c < 2; ++c) {
                const uint64_t *src = a.part + ((size_t)p * a.mchunks * 64 + m) * kRhokRowWords + 3 * c;
                const uint64_t o[3] = {src[0], src[1], src[2]};
                add192(q[c], o);
            }
        std::memcpy(a.row + (size_t)m * kRhokRowWords, q, sizeof q);
    }
    for (int k = 0; k < a.pchunks * a.mchunks; ++k) bad = bad || a.flag[k];
    if (bad) *a.range = 1;
    return hipSuccess;
}

}  // namespace ljmdc

namespace {

// a one-rank system in the engine's layout: T tiles, n live particles scattered over the slots, NaN on the padding
struct System {
    int n, T, P;
    double L;
    std::vector<double> pos;            // [3][P]
    std::vector<int> perm;              // [P] slot -> id; >= n on padding
    std::vector<double> xyz;            // [n][3] in particle order, for the brute force
};

System make_system(int n, int T, double L, unsigned seed)
{
    System s;
    s.n = n; s.T = T; s.P = T * 64 + 64; s.L = L;
    s.pos.assign((size_t)3 * s.P, NAN);
    s.perm.assign((size_t)s.P, 0);
    s.xyz.assign((size_t)3 * n, 0.0);
    std::mt19937_64 rng(seed);
    std::uniform_real_distribution<double> u(-0.2, 1.2);
    std::vector<int> slots((size_t)T * 64);
    for (int k = 0; k < T * 64; ++k) slots[(size_t)k] = k;
    std::shuffle(slots.begin(), slots.end(), rng);
    for (int k = 0; k < s.P; ++k) s.perm[(size_t)k] = n + k;            // padding until a particle takes the slot
    for (int i = 0; i < n; ++i) {
        const int slot = slots[(size_t)i];
        s.perm[(size_t)slot] = i;
        for (int k = 0; k < 3; ++k) {
            const double x = u(rng) * L + (i % 7 == 0 ? 3.0 * L : i % 11 == 0 ? -3.0 * L : 0.0);
            s.pos[(size_t)k * s.P + slot] = x;
            s.xyz[3 * (size_t)i + k] = x;
        }
    }
    return s;
}

ResidentView view_of(const System &s)
{
    ResidentView v;
    v.n = s.n; v.P = s.P; v.TB = s.T; v.T = s.T; v.G = 1; v.rank = 0;
    v.L = s.L; v.invL = 1.0 / s.L;
    v.pos = s.pos.data();
    v.perm = s.perm.data();
    v.stream = nullptr;
    return v;
}

std::vector<int32_t> make_modes(int count, unsigned seed)
{
    std::vector<int32_t> m = {0, 0, 0, 1, 0, 0, -1, 0, 0, -3, 2, 7, 1023, -1023, 1023, 1, 0, 0};
    std::mt19937 rng(seed);
    std::uniform_int_distribution<int> u(-40, 40);
    m.resize((size_t)3 * count);
    for (size_t k = 18; k < m.size(); ++k) m[k] = u(rng);
    return m;
}

// the definition over the particles in particle order
std::vector<int64_t> brute(const System &s, const std::vector<int32_t> &modes, bool &bad)
{
    std::vector<int64_t> out;
    for (size_t m = 0; m < modes.size() / 3; ++m) {
        __int128 re = 0, im = 0;
        for (int i = 0; i < s.n; ++i) add_term(&s.xyz[3 * (size_t)i], &modes[3 * m], s.L, re, im, bad);
        uint64_t q[2][3];
        from128(q[0], re);
        from128(q[1], im);
        for (int c = 0; c < 2; ++c)
            for (int w = 0; w < 3; ++w) out.push_back((int64_t)q[c][w]);
    }
    return out;
}

void guards_and_sequences()
{
    const System s = make_system(300, 8, 10.0, 1);
    const ResidentView v = view_of(s);
    const std::vector<int32_t> modes = make_modes(70, 3);
    RhokState st;
    std::string err;
    std::vector<int64_t> words(4 * 70 * 6, -1);
    std::vector<double> rho(4 * 70 * 2, -1.0);
    int64_t snaps = -1;
    double ms = -1.0;
    const char *who = "caller";

    // before configure
    check(rhok_accumulate(&st, &err, who, v) == LJMD_ERR_STATE && has(err, "caller: the density modes are not configured (call ljmd_rhok_configure first)"),
          "accumulate before configure");
    check(rhok_fetch(&st, &err, who, v, words.data(), &snaps) == LJMD_ERR_STATE && has(err, "not configured"), "read_exact before configure");
    check(rhok_read(&st, &err, who, v, rho.data(), &snaps) == LJMD_ERR_STATE && has(err, "not configured"), "read before configure");
    check(rhok_reset(&st, &err, who, v) == LJMD_ERR_STATE && has(err, "not configured"), "reset before configure");
    check(rhok_profile_read(&st, &err, who, v, &ms) == LJMD_ERR_STATE, "profile_read before configure");
    check(g_terms + g_fold == 0, "nothing launched before configure");
    rhok_release(&st, nullptr);                              // what ljmd_destroy does on a handle never configured

    // guards of configure in their order, each leaving what was there
    ResidentView two = v, multi = v, big = v;
    two.G = 2; two.rank = 1; two.T = 2 * v.TB;
    multi.multi = true; multi.G = 2;
    big.n = kRhokMaxN + 1;
    std::vector<int32_t> over = modes;
    over[3 * 9 + 1] = 1024;
    check(rhok_configure(&st, &err, who, two, 70, modes.data(), -1) == LJMD_ERR_INVALID_ARG &&
              has(err, "caller: max_snapshots = -1 outside 1..262144 (0 switches the density modes off)"), "max_snapshots < 0 comes first");
    check(rhok_configure(&st, &err, who, v, 70, modes.data(), kRhokMaxSnapshots + 1) == LJMD_ERR_INVALID_ARG && has(err, "max_snapshots = 262145"),
          "max_snapshots too large");
    check(rhok_configure(&st, &err, who, two, 0, nullptr, 4) == LJMD_ERR_INVALID_ARG && has(err, "caller: n_ranks = 2: a rank holds only its own particles") &&
              has(err, "one-rank engine (ljmd_create with n_ranks = 1)"), "a rank engine is refused, before the list is looked at");
    check(rhok_configure(&st, &err, who, multi, 70, modes.data(), 4) == LJMD_ERR_INVALID_ARG && has(err, "caller: n_ranks = 2 (multi-device handle): a rank holds"),
          "a multi-device view is refused");
    check(rhok_configure(&st, &err, who, v, 0, modes.data(), 4) == LJMD_ERR_INVALID_ARG && has(err, "caller: n_modes = 0 outside 1..4096"), "n_modes = 0");
    check(rhok_configure(&st, &err, who, v, kRhokMaxModes + 1, modes.data(), 4) == LJMD_ERR_INVALID_ARG && has(err, "n_modes = 4097"), "n_modes too large");
    check(rhok_configure(&st, &err, who, v, 70, nullptr, 4) == LJMD_ERR_INVALID_ARG && has(err, "caller: modes is NULL"), "modes NULL");
    check(rhok_configure(&st, &err, who, v, 70, over.data(), 4) == LJMD_ERR_INVALID_ARG && has(err, "caller: mode 9 = (") &&
              has(err, "1024") && has(err, "an index outside -1023..1023"), "an index beyond the limit");
    over[3 * 9 + 1] = -1024;
    check(rhok_configure(&st, &err, who, v, 70, over.data(), 4) == LJMD_ERR_INVALID_ARG && has(err, "-1024"), "... on the negative side");
    check(rhok_configure(&st, &err, who, v, 70, modes.data(), (1 << 24) / 70 + 1) == LJMD_ERR_INVALID_ARG &&
              has(err, "caller: max_snapshots * n_modes = 16777250 above 16777216"), "the entries limit");
    check(rhok_configure(&st, &err, who, big, 70, modes.data(), 4) == LJMD_ERR_INVALID_ARG && has(err, "caller: n = 8388609 outside 1..8388608"), "n too large");
    check(st.max_snapshots == 0 && !st.d_series && !st.d_part && !st.d_modes, "refused configure allocates nothing");
    check(rhok_configure(&st, &err, who, big, 0, nullptr, 0) == LJMD_OK && rhok_configure(&st, &err, who, two, -7, nullptr, 0) == LJMD_OK &&
              rhok_configure(&st, &err, who, multi, 70, over.data(), 0) == LJMD_OK, "off needs no valid list, n or one-rank engine");

    std::vector<int32_t> gone = modes;                       // the list is copied: the caller's may change afterwards
    check(rhok_configure(&st, &err, who, v, 70, gone.data(), 3) == LJMD_OK && st.max_snapshots == 3 && st.n_modes == 70 && st.d_series &&
              st.d_part && st.d_modes && st.d_flag && st.d_range && st.plan.mchunks == 2 && st.plan.pchunks == 8 && st.plan.tiles == 1,
          "configure");
    std::fill(gone.begin(), gone.end(), 77);
    check(rhok_configure(&st, &err, who, v, 70, modes.data(), -5) == LJMD_ERR_INVALID_ARG && st.max_snapshots == 3, "a refused reconfigure keeps the configuration");
    check(rhok_configure(&st, &err, who, multi, 70, modes.data(), 2) == LJMD_ERR_INVALID_ARG && st.max_snapshots == 3, "... for the rank guard too");
    check(rhok_configure(&st, &err, who, v, 70, over.data(), 2) == LJMD_ERR_INVALID_ARG && st.max_snapshots == 3 && st.d_series, "... and the index guard");
    check(rhok_fetch(&st, &err, who, v, words.data(), &snaps) == LJMD_OK && snaps == 0 && words[0] == -1, "an empty series copies nothing");
    check(rhok_profile_read(&st, &err, who, v, &ms) == LJMD_OK && ms == 0.0, "profile before the first accumulate");

    // the words against brute force
    bool bad = false;
    const std::vector<int64_t> want = brute(s, modes, bad);
    check(!bad, "the test system is in range");
    check(rhok_accumulate(&st, &err, who, v) == LJMD_OK && g_terms == 1 && g_fold == 1, "accumulate: two launches");
    check(g_last.pos == v.pos && g_last.perm == v.perm && g_last.modes == st.d_modes && g_last.L == 10.0 && g_last.T == 8 && g_last.P == s.P &&
              g_last.n == 300 && g_last.n_modes == 70, "accumulate: arguments");
    check(rhok_fetch(&st, &err, who, v, words.data(), &snaps) == LJMD_OK && snaps == 1 &&
              std::memcmp(words.data(), want.data(), want.size() * sizeof(int64_t)) == 0, "one snapshot equals the brute-force sum");
    check(words[70 * 6] == -1, "read_exact writes the taken snapshots only");
    check(words[0] == 0 && words[1] == 300 && words[2] == 0 && words[3] == 0 && words[4] == 0 && words[5] == 0, "mode (0, 0, 0): Re = n 2^64, Im = 0");
    check(std::memcmp(&words[6], &words[12], 3 * sizeof(int64_t)) == 0, "mode -n: the same Re words");
    {
        uint64_t a[3] = {(uint64_t)words[9], (uint64_t)words[10], (uint64_t)words[11]};
        const uint64_t b[3] = {(uint64_t)words[15], (uint64_t)words[16], (uint64_t)words[17]};
        add192(a, b);
        check(a[0] == 0 && a[1] == 0 && a[2] == 0 && (words[9] != 0 || words[10] != 0), "mode -n: exactly negated Im words");
    }
    check(std::memcmp(&words[6], &words[30], 6 * sizeof(int64_t)) == 0, "a duplicate mode has the same words");
    check(rhok_profile_read(&st, &err, who, v, nullptr) == LJMD_OK, "profile with a NULL pointer");
    check(rhok_fetch(&st, &err, who, v, nullptr, nullptr) == LJMD_OK && rhok_read(&st, &err, who, v, nullptr, nullptr) == LJMD_OK, "reads with NULL pointers");

    // doubles: one rounding of each integer
    check(rhok_read(&st, &err, who, v, rho.data(), &snaps) == LJMD_OK && snaps == 1 && rho[70 * 2] == -1.0, "read");
    bool same = true;
    for (int k = 0; k < 70 * 2; ++k) {
        const uint64_t u[3] = {(uint64_t)words[3 * k], (uint64_t)words[3 * k + 1], (uint64_t)words[3 * k + 2]};
        const double d = ljmdk::fixed_to_double(u);
        same = same && std::memcmp(&d, &rho[(size_t)k], sizeof d) == 0;
    }
    check(same && rho[0] == 300.0 && rho[1] == 0.0, "read = fixed_to_double of read_exact");

    // a second row; a failed launch: reported, not counted
    check(rhok_accumulate(&st, &err, who, v) == LJMD_OK && rhok_fetch(&st, &err, who, v, words.data(), &snaps) == LJMD_OK && snaps == 2 &&
              std::memcmp(words.data() + 70 * 6, want.data(), want.size() * sizeof(int64_t)) == 0, "the second row equals the first");
    g_fail_terms = 1;
    check(rhok_accumulate(&st, &err, who, v) == LJMD_ERR_HIP && has(err, "caller: density modes launch failed"), "failed launch");
    check(rhok_fetch(&st, &err, who, v, nullptr, &snaps) == LJMD_OK && snaps == 2, "failed launch adds no snapshot");

    // a full series
    check(rhok_accumulate(&st, &err, who, v) == LJMD_OK, "third snapshot");
    const int launches = g_terms + g_fold;
    check(rhok_accumulate(&st, &err, who, v) == LJMD_ERR_STATE && has(err, "caller: the series is full (3 snapshots") && has(err, "ljmd_rhok_reset"),
          "full series");
    check(g_terms + g_fold == launches, "a full series launches nothing");
    check(rhok_fetch(&st, &err, who, v, words.data(), &snaps) == LJMD_OK && snaps == 3, "full series reads");
    check(rhok_reset(&st, &err, who, v) == LJMD_OK && rhok_fetch(&st, &err, who, v, nullptr, &snaps) == LJMD_OK && snaps == 0, "reset empties");
    check(rhok_accumulate(&st, &err, who, v) == LJMD_OK, "room again after reset");

    // an engine of another shape, or of more ranks
    const System other = make_system(600, 12, 10.0, 2);
    check(rhok_accumulate(&st, &err, who, view_of(other)) == LJMD_ERR_STATE && has(err, "not the one the density modes were configured for"),
          "a view of another shape is refused");
    ResidentView ranked = v;
    ranked.G = 2;
    const int before = g_terms;
    check(rhok_accumulate(&st, &err, who, ranked) == LJMD_ERR_STATE && g_terms == before, "a rank view never reaches the kernels");

    // reconfigure empties, off frees
    check(rhok_configure(&st, &err, who, v, 5, modes.data(), 2) == LJMD_OK && st.max_snapshots == 2 && st.n_modes == 5 && st.snapshots == 0, "reconfigure");
    check(rhok_accumulate(&st, &err, who, v) == LJMD_OK && rhok_fetch(&st, &err, who, v, words.data(), &snaps) == LJMD_OK && snaps == 1 &&
              std::memcmp(words.data(), want.data(), 5 * 6 * sizeof(int64_t)) == 0, "a shorter list: the same words per mode");
    check(rhok_configure(&st, &err, who, v, 0, nullptr, 0) == LJMD_OK && st.max_snapshots == 0 && !st.d_series && !st.d_part && !st.d_modes &&
              !st.d_flag && !st.d_range && !st.timer.ev0 && !st.timer.ev1, "off frees");
    check(rhok_accumulate(&st, &err, who, v) == LJMD_ERR_STATE && rhok_fetch(&st, &err, who, v, nullptr, nullptr) == LJMD_ERR_STATE, "off: as before configure");
    check(rhok_configure(&st, &err, who, v, 70, modes.data(), 2) == LJMD_OK && rhok_accumulate(&st, &err, who, v) == LJMD_OK, "configured again");
    rhok_release(&st, nullptr);                              // what ljmd_destroy does on a configured handle
    check(st.max_snapshots == 0 && !st.d_series, "release");
    rhok_release(&st, nullptr);
}

// one partly filled chunk in both directions, whole chunks, many tiles per particle chunk: always the brute-force integers
void grids_against_brute_force()
{
    struct Case { int n, T, modes; };
    const Case cases[] = {{108, 2, 6}, {64, 1, 64}, {2, 1, 65}, {500, 8, 257}, {700, 11, 128}, {3000, 47, 7}, {70000, 1100, 6}};
    for (const Case &c : cases) {
        const System s = make_system(c.n, c.T, 68.94, 100 + (unsigned)c.n);
        const ResidentView v = view_of(s);
        const std::vector<int32_t> modes = make_modes(c.modes, (unsigned)c.modes);
        RhokState st;
        std::string err;
        bool bad = false;
        const std::vector<int64_t> want = brute(s, modes, bad);
        std::vector<int64_t> got(want.size(), -1);
        check(rhok_configure(&st, &err, "w", v, c.modes, modes.data(), 1) == LJMD_OK && rhok_accumulate(&st, &err, "w", v) == LJMD_OK &&
                  rhok_fetch(&st, &err, "w", v, got.data(), nullptr) == LJMD_OK && got == want, "the grid equals the brute-force sum");
        check(g_last.pchunks * g_last.tiles >= c.T && g_last.pchunks <= kRhokMaxChunks, "the plan covers the tiles");
        check(!bad, "grid cases are in range");
        rhok_release(&st, nullptr);
    }
    const RhokPlan big = rhok_plan(4096, 1024), few = rhok_plan(4096, 64), most = rhok_plan(4096, 4096), wide = rhok_plan(1 << 17, 1);
    check(big.mchunks == 16 && big.tiles == 8 && big.pchunks == 512, "plan: N = 262144, 1024 modes: 8192 units");
    check(few.mchunks == 1 && few.tiles == 4 && few.pchunks == 1024, "plan: 64 modes: the chunk limit");
    check(most.mchunks == 64 && most.tiles == 32 && most.pchunks == 128, "plan: 4096 modes");
    check(wide.pchunks == 1024 && wide.tiles == 128, "plan: n = 2^23");
}

// a NaN coordinate on one live particle: its terms enter as 0, the sticky word is set until reset; padding sets nothing
void range_flag()
{
    System s = make_system(128, 3, 10.0, 9);
    const std::vector<int32_t> modes = make_modes(6, 1);
    const ResidentView v = view_of(s);
    RhokState st;
    std::string err;
    int64_t snaps = -1;
    bool bad = false;
    std::vector<int64_t> want = brute(s, modes, bad), got(want.size(), -1);
    check(!bad, "NaN on the padding slots alone sets no flag in the brute force");
    check(rhok_configure(&st, &err, "g", v, 6, modes.data(), 4) == LJMD_OK && rhok_accumulate(&st, &err, "g", v) == LJMD_OK &&
              rhok_fetch(&st, &err, "g", v, got.data(), &snaps) == LJMD_OK && got == want && got[1] == 128, "padding adds nothing and sets no flag");
    const int slot = (int)(std::find(s.perm.begin(), s.perm.end(), 5) - s.perm.begin());
    s.pos[(size_t)s.P + slot] = NAN;
    s.xyz[3 * 5 + 1] = NAN;
    want = brute(s, modes, bad);
    check(bad, "a NaN coordinate is out of range");
    snaps = -1;
    check(rhok_accumulate(&st, &err, "g", v) == LJMD_OK, "accumulate succeeds");
    got.assign(2 * want.size(), -1);
    check(rhok_fetch(&st, &err, "g", v, got.data(), &snaps) == LJMD_ERR_RANGE && has(err, "g: a particle's density mode terms were not finite") &&
              has(err, "until ljmd_rhok_reset") && snaps == -1, "read_exact: LJMD_ERR_RANGE");
    check(std::memcmp(got.data() + want.size(), want.data(), want.size() * sizeof(int64_t)) == 0 && got[want.size() + 1] == 127,
          "the flagged particle entered as zeros, everything else as usual");
    double rho[24];
    check(rhok_read(&st, &err, "g", v, rho, nullptr) == LJMD_ERR_RANGE, "read: LJMD_ERR_RANGE");
    s.pos[(size_t)s.P + slot] = 1.0;
    check(rhok_accumulate(&st, &err, "g", v) == LJMD_OK && rhok_fetch(&st, &err, "g", v, nullptr, nullptr) == LJMD_ERR_RANGE, "sticky");
    check(rhok_reset(&st, &err, "g", v) == LJMD_OK && rhok_fetch(&st, &err, "g", v, nullptr, &snaps) == LJMD_OK && snaps == 0, "reset clears the word");
    // L not finite: every term
    ResidentView w = v;
    w.L = INFINITY;
    check(rhok_accumulate(&st, &err, "g", w) == LJMD_OK && rhok_fetch(&st, &err, "g", w, nullptr, nullptr) == LJMD_OK,
          "L = inf: every coordinate is 0 turns, in range");
    w.L = NAN;
    check(rhok_accumulate(&st, &err, "g", w) == LJMD_OK && rhok_fetch(&st, &err, "g", w, nullptr, nullptr) == LJMD_ERR_RANGE, "L = NaN sets the word");
    rhok_release(&st, nullptr);
}

void select_modes()
{
    int32_t m[64 * 3], count = -1;
    check(ljmd_rhok_select_modes(1, 8, 64, m, &count) == LJMD_OK && count == 3 && m[0] == 0 && m[1] == 0 && m[2] == 1 && m[3] == 0 && m[4] == 1 &&
              m[5] == 0 && m[6] == 1 && m[7] == 0 && m[8] == 0, "select_modes: |n|^2 = 1");
    check(ljmd_rhok_select_modes(3, 2, 64, m, &count) == LJMD_OK && count == 6 && m[6] == 0 && m[7] == 1 && m[8] == -1 && m[9] == 1 && m[10] == 0 &&
              m[11] == -1 && m[12] == 1 && m[13] == -1 && m[14] == -1 && m[15] == 1 && m[16] == 1 && m[17] == -1,
          "select_modes: members floor(j count / per_shell) of a shell");
    m[15] = 99;
    check(ljmd_rhok_select_modes(3, 2, 5, m, &count) == LJMD_ERR_INVALID_ARG && count == 6 && m[15] == 99 &&
              has(ljmdh::g_last_error, "ljmd_rhok_select_modes: capacity = 5 too small: 6 modes"), "select_modes: capacity");
    check(ljmd_rhok_select_modes(3, 2, 0, nullptr, &count) == LJMD_ERR_INVALID_ARG && count == 6, "select_modes: the count alone");
    check(ljmd_rhok_select_modes(0, 2, 64, m, &count) == LJMD_ERR_INVALID_ARG && ljmd_rhok_select_modes(3, 0, 64, m, &count) == LJMD_ERR_INVALID_ARG &&
              ljmd_rhok_select_modes(3, 2, 64, nullptr, &count) == LJMD_ERR_INVALID_ARG && ljmd_rhok_select_modes(3, 2, 64, m, nullptr) == LJMD_ERR_INVALID_ARG &&
              ljmd_rhok_select_modes(3, 2, -1, m, &count) == LJMD_ERR_INVALID_ARG, "select_modes: guards");
}

}  // namespace

int main()
{
    setenv("FAKEHIP_DEVICES", "1", 1);
    guards_and_sequences();
    grids_against_brute_force();
    range_flag();
    select_modes();
    if (g_failures == 0) std::printf("rhok_host: ok\n");
    return g_failures == 0 ? 0 : 1;
}
