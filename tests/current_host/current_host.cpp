// current_host.cpp -- TEST INFRASTRUCTURE: the host core of the engine's resident current modes (csrc/ljmd_current.cpp,
// namespace ljmdc) without a GPU and without the engine.  Linked from the core, ljmd_common.cpp, the fake HIP runtime
// (tests/fakehip) and its own definitions of the two launchers, which check what they are given and carry out on the
// host what the kernels mean through ljmd_current_arith.h: units of (particle chunk, mode chunk), live slots by the
// permutation, rows of partials with their padding, flags, and the fold.  The program checks itself -- every guard with
// its return code and message in order, the refusal of rank engines and multi-device views, the sequences around
// configure / accumulate / read / reset, a full series, the entries limit, NULL outputs, release while configured, the
// range word, and the returned words against a brute-force sum over the particles in particle order -- prints one line
// per check that fails and "current_host: ok" when none did.  It also prints one system, its mode list and the words it
// read ("L", "particle", "mode", "words" lines, doubles in hexadecimal), which tests/test_current_host.py compares with
// tests/current_model.py; the test runs it under ASan and UBSan.
// (The fake hipMalloc cannot fail, so the LJMD_ERR_ALLOC branch of configure is not reached here.)
#include "ljmd.h"
#include "ljmd_current_arith.h"
#include "ljmd_internal.h"
#include "ljmd_resident.h"

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
CurrentTermsArgs g_last{};

void check(bool ok, const char *what)
{
    if (ok) return;
    ++g_failures;
    std::printf("FAILED: %s\n", what);
}

bool has(const std::string &err, const char *text) { return err.find(text) != std::string::npos; }

// the definition's term of particle (x, v) and mode n into the six sums
void add_term(const double *x, const double *vel, const int32_t *n, double L, __int128 (&acc)[6], bool &bad)
{
    double C, S, t[6];
    ljmdk::rhok_term((double)n[0], (double)n[1], (double)n[2], ljmdk::rhok_turns(x[0], L), ljmdk::rhok_turns(x[1], L),
                     ljmdk::rhok_turns(x[2], L), C, S);
    ljmdk::current_products(vel[0], vel[1], vel[2], C, S, t);
    const bool oob = ljmdk::current_out_of_range(C, S, t);
    bad = bad || oob;
    for (int k = 0; k < 6; ++k) ljmdk::current_fixed_add(acc[k], oob ? 0.0 : t[k]);
}

}  // namespace

namespace ljmdc {

// current_terms_kernel on the host: unit by unit, lane by lane
hipError_t launch_current_terms(const CurrentTermsArgs &a, hipStream_t)
{
    ++g_terms;
    if (g_fail_terms > 0 && --g_fail_terms == 0) return hipErrorLaunchFailure;
    g_last = a;
    check(current_terms_ok(a), "terms launch: arguments");
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
            __int128 acc[6] = {0, 0, 0, 0, 0, 0};
            bool bad = false;
            for (int t = pc * a.tiles; t < std::min(a.T, (pc + 1) * a.tiles); ++t)
                for (int j = 0; j < 64; ++j) {
                    const size_t s = (size_t)t * 64 + j;
                    if (a.perm[s] < 0 || a.perm[s] >= a.n) continue;
                    const double x[3] = {a.pos[s], a.pos[P + s], a.pos[2 * P + s]};
                    const double w[3] = {a.v[s], a.v[P + s], a.v[2 * P + s]};
                    add_term(x, w, n, a.L, acc, bad);
                }
            uint64_t q[6][3] = {};
            if (mode_live)
                for (int k = 0; k < 6; ++k) from128(q[k], acc[k]);
            std::memcpy(a.part + ((size_t)pc * a.mchunks * 64 + m) * kCurrentRowWords, q, sizeof q);
            any_bad = any_bad || (bad && mode_live);
        }
        a.flag[(size_t)pc * a.mchunks + y] = any_bad ? 1u : 0u;
    }
    return hipSuccess;
}

hipError_t launch_current_fold(const CurrentFoldArgs &a, hipStream_t)
{
    ++g_fold;
    check(current_fold_ok(a), "fold launch: arguments");
    bool bad = false;
    for (int m = 0; m < a.n_modes; ++m) {
        uint64_t q[6][3] = {};
        for (int p = 0; p < a.pchunks; ++p)
            for (int c = 0; c < 6; ++c) {
                const uint64_t *src = a.part + ((size_t)p * a.mchunks * 64 + m) * kCurrentRowWords + 3 * c;
                const uint64_t o[3] = {src[0], src[1], src[2]};
                add192(q[c], o);
            }
        std::memcpy(a.row + (size_t)m * kCurrentRowWords, q, sizeof q);
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
    std::vector<double> pos, vel;       // [3][P]
    std::vector<int> perm;              // [P] slot -> id; >= n on padding
    std::vector<double> xyz, vxyz;      // [n][3] in particle order, for the brute force
};

System make_system(int n, int T, double L, unsigned seed)
{
    System s;
    s.n = n; s.T = T; s.P = T * 64 + 64; s.L = L;
    s.pos.assign((size_t)3 * s.P, NAN);
    s.vel.assign((size_t)3 * s.P, NAN);
    s.perm.assign((size_t)s.P, 0);
    s.xyz.assign((size_t)3 * n, 0.0);
    s.vxyz.assign((size_t)3 * n, 0.0);
    std::mt19937_64 rng(seed);
    std::uniform_real_distribution<double> u(-0.2, 1.2), w(-3.0, 3.0);
    std::vector<int> slots((size_t)T * 64);
    for (int k = 0; k < T * 64; ++k) slots[(size_t)k] = k;
    std::shuffle(slots.begin(), slots.end(), rng);
    for (int k = 0; k < s.P; ++k) s.perm[(size_t)k] = n + k;            // padding until a particle takes the slot
    for (int i = 0; i < n; ++i) {
        const int slot = slots[(size_t)i];
        s.perm[(size_t)slot] = i;
        for (int k = 0; k < 3; ++k) {
            const double x = u(rng) * L + (i % 7 == 0 ? 3.0 * L : i % 11 == 0 ? -3.0 * L : 0.0);
            const double vv = w(rng);
            s.pos[(size_t)k * s.P + slot] = x;
            s.vel[(size_t)k * s.P + slot] = vv;
            s.xyz[3 * (size_t)i + k] = x;
            s.vxyz[3 * (size_t)i + k] = vv;
        }
    }
    return s;
}

void set_velocity(System &s, int id, int axis, double value)
{
    const int slot = (int)(std::find(s.perm.begin(), s.perm.end(), id) - s.perm.begin());
    s.vel[(size_t)axis * s.P + slot] = value;
    s.vxyz[3 * (size_t)id + axis] = value;
}

ResidentView view_of(const System &s)
{
    ResidentView v;
    v.n = s.n; v.P = s.P; v.TB = s.T; v.T = s.T; v.G = 1; v.rank = 0;
    v.L = s.L; v.invL = 1.0 / s.L;
    v.pos = s.pos.data();
    v.v = s.vel.data();
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
        __int128 acc[6] = {0, 0, 0, 0, 0, 0};
        for (int i = 0; i < s.n; ++i) add_term(&s.xyz[3 * (size_t)i], &s.vxyz[3 * (size_t)i], &modes[3 * m], s.L, acc, bad);
        for (int c = 0; c < 6; ++c) {
            uint64_t q[3];
            from128(q, acc[c]);
            for (int w = 0; w < 3; ++w) out.push_back((int64_t)q[w]);
        }
    }
    return out;
}

bool negated(const int64_t *a, const int64_t *b)
{
    uint64_t x[3] = {(uint64_t)a[0], (uint64_t)a[1], (uint64_t)a[2]};
    const uint64_t y[3] = {(uint64_t)b[0], (uint64_t)b[1], (uint64_t)b[2]};
    add192(x, y);
    return x[0] == 0 && x[1] == 0 && x[2] == 0;
}

constexpr int W = kCurrentRowWords;     // 18

void guards_and_sequences()
{
    const System s = make_system(300, 8, 10.0, 1);
    const ResidentView v = view_of(s);
    const std::vector<int32_t> modes = make_modes(70, 3);
    CurrentState st;
    std::string err;
    std::vector<int64_t> words(4 * 70 * W, -1);
    std::vector<double> j(4 * 70 * 6, -1.0);
    int64_t snaps = -1;
    double ms = -1.0;
    const char *who = "caller";

    // before configure
    check(current_accumulate(&st, &err, who, v) == LJMD_ERR_STATE &&
              has(err, "caller: the current modes are not configured (call ljmd_current_configure first)"), "accumulate before configure");
    check(current_fetch(&st, &err, who, v, words.data(), &snaps) == LJMD_ERR_STATE && has(err, "not configured"), "read_exact before configure");
    check(current_read(&st, &err, who, v, j.data(), &snaps) == LJMD_ERR_STATE && has(err, "not configured"), "read before configure");
    check(current_reset(&st, &err, who, v) == LJMD_ERR_STATE && has(err, "not configured"), "reset before configure");
    check(current_profile_read(&st, &err, who, v, &ms) == LJMD_ERR_STATE, "profile_read before configure");
    check(g_terms + g_fold == 0, "nothing launched before configure");
    current_release(&st, nullptr);                           // what ljmd_destroy does on a handle never configured

    // guards of configure in their order, each leaving what was there
    ResidentView two = v, multi = v, big = v;
    two.G = 2; two.rank = 1; two.T = 2 * v.TB;
    multi.multi = true; multi.G = 2;
    big.n = kRhokMaxN + 1;
    std::vector<int32_t> over = modes;
    over[3 * 9 + 1] = 1024;
    check(current_configure(&st, &err, who, two, 70, modes.data(), -1) == LJMD_ERR_INVALID_ARG &&
              has(err, "caller: max_snapshots = -1 outside 1..262144 (0 switches the current modes off)"), "max_snapshots < 0 comes first");
    check(current_configure(&st, &err, who, v, 70, modes.data(), kCurrentMaxSnapshots + 1) == LJMD_ERR_INVALID_ARG && has(err, "max_snapshots = 262145"),
          "max_snapshots too large");
    check(current_configure(&st, &err, who, two, 0, nullptr, 4) == LJMD_ERR_INVALID_ARG && has(err, "caller: n_ranks = 2: a rank holds only its own particles") &&
              has(err, "one-rank engine (ljmd_create with n_ranks = 1)"), "a rank engine is refused, before the list is looked at");
    check(current_configure(&st, &err, who, multi, 70, modes.data(), 4) == LJMD_ERR_INVALID_ARG &&
              has(err, "caller: n_ranks = 2 (multi-device handle): a rank holds"), "a multi-device view is refused");
    check(current_configure(&st, &err, who, v, 0, modes.data(), 4) == LJMD_ERR_INVALID_ARG && has(err, "caller: n_modes = 0 outside 1..4096"), "n_modes = 0");
    check(current_configure(&st, &err, who, v, kRhokMaxModes + 1, modes.data(), 4) == LJMD_ERR_INVALID_ARG && has(err, "n_modes = 4097"), "n_modes too large");
    check(current_configure(&st, &err, who, v, 70, nullptr, 4) == LJMD_ERR_INVALID_ARG && has(err, "caller: modes is NULL"), "modes NULL");
    check(current_configure(&st, &err, who, v, 70, over.data(), 4) == LJMD_ERR_INVALID_ARG && has(err, "caller: mode 9 = (") && has(err, "1024") &&
              has(err, "an index outside -1023..1023"), "an index beyond the limit");
    over[3 * 9 + 1] = -1024;
    check(current_configure(&st, &err, who, v, 70, over.data(), 4) == LJMD_ERR_INVALID_ARG && has(err, "-1024"), "... on the negative side");
    check(current_configure(&st, &err, who, v, 70, modes.data(), (1 << 22) / 70 + 1) == LJMD_ERR_INVALID_ARG &&
              has(err, "caller: max_snapshots * n_modes = 4194330 above 4194304"), "the entries limit");
    check(current_configure(&st, &err, who, big, 70, modes.data(), 4) == LJMD_ERR_INVALID_ARG && has(err, "caller: n = 8388609 outside 1..8388608"), "n too large");
    check(st.max_snapshots == 0 && !st.d_series && !st.d_part && !st.d_modes, "refused configure allocates nothing");
    check(current_configure(&st, &err, who, big, 0, nullptr, 0) == LJMD_OK && current_configure(&st, &err, who, two, -7, nullptr, 0) == LJMD_OK &&
              current_configure(&st, &err, who, multi, 70, over.data(), 0) == LJMD_OK, "off needs no valid list, n or one-rank engine");

    std::vector<int32_t> gone = modes;                       // the list is copied: the caller's may change afterwards
    check(current_configure(&st, &err, who, v, 70, gone.data(), 3) == LJMD_OK && st.max_snapshots == 3 && st.n_modes == 70 && st.d_series &&
              st.d_part && st.d_modes && st.d_flag && st.d_range && st.plan.mchunks == 2 && st.plan.pchunks == 8 && st.plan.tiles == 1,
          "configure");
    std::fill(gone.begin(), gone.end(), 77);
    check(current_configure(&st, &err, who, v, 70, modes.data(), -5) == LJMD_ERR_INVALID_ARG && st.max_snapshots == 3, "a refused reconfigure keeps the configuration");
    check(current_configure(&st, &err, who, multi, 70, modes.data(), 2) == LJMD_ERR_INVALID_ARG && st.max_snapshots == 3, "... for the rank guard too");
    check(current_configure(&st, &err, who, v, 70, over.data(), 2) == LJMD_ERR_INVALID_ARG && st.max_snapshots == 3 && st.d_series, "... and the index guard");
    check(current_fetch(&st, &err, who, v, words.data(), &snaps) == LJMD_OK && snaps == 0 && words[0] == -1, "an empty series copies nothing");
    check(current_profile_read(&st, &err, who, v, &ms) == LJMD_OK && ms == 0.0, "profile before the first accumulate");

    // the words against brute force
    bool bad = false;
    const std::vector<int64_t> want = brute(s, modes, bad);
    check(!bad, "the test system is in range");
    check(current_accumulate(&st, &err, who, v) == LJMD_OK && g_terms == 1 && g_fold == 1, "accumulate: two launches");
    check(g_last.pos == v.pos && g_last.v == v.v && g_last.perm == v.perm && g_last.modes == st.d_modes && g_last.L == 10.0 && g_last.T == 8 &&
              g_last.P == s.P && g_last.n == 300 && g_last.n_modes == 70, "accumulate: arguments");
    check(current_fetch(&st, &err, who, v, words.data(), &snaps) == LJMD_OK && snaps == 1 &&
              std::memcmp(words.data(), want.data(), want.size() * sizeof(int64_t)) == 0, "one snapshot equals the brute-force sum");
    check(words[70 * W] == -1, "read_exact writes the taken snapshots only");
    {
        // mode (0, 0, 0): Re_a = sum Q(v_a), Im_a = 0
        bool ok = true;
        for (int a = 0; a < 3; ++a) {
            __int128 sum = 0;
            for (int i = 0; i < s.n; ++i) ljmdk::current_fixed_add(sum, s.vxyz[3 * (size_t)i + a]);
            uint64_t q[3];
            from128(q, sum);
            for (int w = 0; w < 3; ++w) ok = ok && (uint64_t)words[6 * a + w] == q[w] && words[6 * a + 3 + w] == 0;
        }
        check(ok, "mode (0, 0, 0): the total momentum, Im = 0");
    }
    {
        bool ok = true, some = false;
        for (int a = 0; a < 3; ++a) {
            ok = ok && std::memcmp(&words[W + 6 * a], &words[2 * W + 6 * a], 3 * sizeof(int64_t)) == 0;
            ok = ok && negated(&words[W + 6 * a + 3], &words[2 * W + 6 * a + 3]);
            some = some || words[W + 6 * a + 3] != 0;
        }
        check(ok && some, "mode -n: the same Re words, exactly negated Im words");
    }
    check(std::memcmp(&words[W], &words[5 * W], W * sizeof(int64_t)) == 0, "a duplicate mode has the same words");
    check(current_profile_read(&st, &err, who, v, nullptr) == LJMD_OK, "profile with a NULL pointer");
    check(current_fetch(&st, &err, who, v, nullptr, nullptr) == LJMD_OK && current_read(&st, &err, who, v, nullptr, nullptr) == LJMD_OK,
          "reads with NULL pointers");

    // doubles: one rounding of each integer
    check(current_read(&st, &err, who, v, j.data(), &snaps) == LJMD_OK && snaps == 1 && j[70 * 6] == -1.0, "read");
    bool same = true;
    for (int k = 0; k < 70 * 6; ++k) {
        const uint64_t u[3] = {(uint64_t)words[3 * k], (uint64_t)words[3 * k + 1], (uint64_t)words[3 * k + 2]};
        const double d = ljmdk::fixed_to_double(u);
        same = same && std::memcmp(&d, &j[(size_t)k], sizeof d) == 0;
    }
    check(same && j[1] == 0.0, "read = fixed_to_double of read_exact");

    // a second row; a failed launch: reported, not counted
    check(current_accumulate(&st, &err, who, v) == LJMD_OK && current_fetch(&st, &err, who, v, words.data(), &snaps) == LJMD_OK && snaps == 2 &&
              std::memcmp(words.data() + 70 * W, want.data(), want.size() * sizeof(int64_t)) == 0, "the second row equals the first");
    g_fail_terms = 1;
    check(current_accumulate(&st, &err, who, v) == LJMD_ERR_HIP && has(err, "caller: current modes launch failed"), "failed launch");
    check(current_fetch(&st, &err, who, v, nullptr, &snaps) == LJMD_OK && snaps == 2, "failed launch adds no snapshot");

    // a full series
    check(current_accumulate(&st, &err, who, v) == LJMD_OK, "third snapshot");
    const int launches = g_terms + g_fold;
    check(current_accumulate(&st, &err, who, v) == LJMD_ERR_STATE && has(err, "caller: the series is full (3 snapshots") &&
              has(err, "ljmd_current_reset"), "full series");
    check(g_terms + g_fold == launches, "a full series launches nothing");
    check(current_fetch(&st, &err, who, v, words.data(), &snaps) == LJMD_OK && snaps == 3, "full series reads");
    check(current_reset(&st, &err, who, v) == LJMD_OK && current_fetch(&st, &err, who, v, nullptr, &snaps) == LJMD_OK && snaps == 0, "reset empties");
    check(current_accumulate(&st, &err, who, v) == LJMD_OK, "room again after reset");

    // an engine of another shape, of more ranks, or without velocities
    const System other = make_system(600, 12, 10.0, 2);
    check(current_accumulate(&st, &err, who, view_of(other)) == LJMD_ERR_STATE && has(err, "not the one the current modes were configured for"),
          "a view of another shape is refused");
    ResidentView ranked = v, bare = v;
    ranked.G = 2;
    bare.v = nullptr;
    const int before = g_terms;
    check(current_accumulate(&st, &err, who, ranked) == LJMD_ERR_STATE && g_terms == before, "a rank view never reaches the kernels");
    check(current_accumulate(&st, &err, who, bare) == LJMD_ERR_STATE && g_terms == before, "nor does a view without velocities");

    // reconfigure empties, off frees
    check(current_configure(&st, &err, who, v, 5, modes.data(), 2) == LJMD_OK && st.max_snapshots == 2 && st.n_modes == 5 && st.snapshots == 0, "reconfigure");
    check(current_accumulate(&st, &err, who, v) == LJMD_OK && current_fetch(&st, &err, who, v, words.data(), &snaps) == LJMD_OK && snaps == 1 &&
              std::memcmp(words.data(), want.data(), 5 * W * sizeof(int64_t)) == 0, "a shorter list: the same words per mode");
    check(current_configure(&st, &err, who, v, 0, nullptr, 0) == LJMD_OK && st.max_snapshots == 0 && !st.d_series && !st.d_part && !st.d_modes &&
              !st.d_flag && !st.d_range && !st.timer.ev0 && !st.timer.ev1, "off frees");
    check(current_accumulate(&st, &err, who, v) == LJMD_ERR_STATE && current_fetch(&st, &err, who, v, nullptr, nullptr) == LJMD_ERR_STATE,
          "off: as before configure");
    check(current_configure(&st, &err, who, v, 70, modes.data(), 2) == LJMD_OK && current_accumulate(&st, &err, who, v) == LJMD_OK, "configured again");
    current_release(&st, nullptr);                           // what ljmd_destroy does on a configured handle
    check(st.max_snapshots == 0 && !st.d_series, "release");
    current_release(&st, nullptr);
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
        CurrentState st;
        std::string err;
        bool bad = false;
        const std::vector<int64_t> want = brute(s, modes, bad);
        std::vector<int64_t> got(want.size(), -1);
        check(current_configure(&st, &err, "w", v, c.modes, modes.data(), 1) == LJMD_OK && current_accumulate(&st, &err, "w", v) == LJMD_OK &&
                  current_fetch(&st, &err, "w", v, got.data(), nullptr) == LJMD_OK && got == want, "the grid equals the brute-force sum");
        check(g_last.pchunks * g_last.tiles >= c.T && g_last.pchunks <= kRhokMaxChunks, "the plan covers the tiles");
        check(!bad, "grid cases are in range");
        current_release(&st, nullptr);
    }
}

// velocities at the bound, NaN and infinite, and a NaN coordinate: the whole (particle, mode) term enters as zeros, the
// sticky word is set until reset; padding sets nothing
void range_flag()
{
    System s = make_system(128, 3, 10.0, 9);
    const std::vector<int32_t> modes = make_modes(6, 1);
    const ResidentView v = view_of(s);
    CurrentState st;
    std::string err;
    int64_t snaps = -1;
    bool bad = false;
    std::vector<int64_t> want = brute(s, modes, bad), got(want.size(), -1);
    check(!bad, "NaN on the padding slots alone sets no flag in the brute force");
    check(current_configure(&st, &err, "g", v, 6, modes.data(), 8) == LJMD_OK && current_accumulate(&st, &err, "g", v) == LJMD_OK &&
              current_fetch(&st, &err, "g", v, got.data(), &snaps) == LJMD_OK && got == want, "padding adds nothing and sets no flag");
    struct Fault { int id, axis; double value; };
    const Fault faults[] = {{5, 0, 0x1p40}, {6, 1, NAN}, {7, 2, INFINITY}};
    for (const Fault &f : faults) {
        const double keep = s.vxyz[3 * (size_t)f.id + f.axis];
        set_velocity(s, f.id, f.axis, f.value);
        bad = false;
        want = brute(s, modes, bad);
        check(bad, "the velocity is out of range");
        check(current_reset(&st, &err, "g", v) == LJMD_OK && current_accumulate(&st, &err, "g", v) == LJMD_OK, "accumulate succeeds");
        got.assign(want.size(), -1);
        snaps = -1;
        check(current_fetch(&st, &err, "g", v, got.data(), &snaps) == LJMD_ERR_RANGE && has(err, "g: a particle's current mode terms were not finite or reached 2^40") &&
                  has(err, "until ljmd_current_reset") && snaps == -1, "read_exact: LJMD_ERR_RANGE");
        check(got == want, "the flagged terms entered as zeros, everything else as usual");
        set_velocity(s, f.id, f.axis, keep);
    }
    // 2^40 times a cosine below 1 is in range: only the modes whose C or S make the product reach the bound are dropped
    {
        set_velocity(s, 5, 0, 0x1p40);
        System lone = s;
        set_velocity(lone, 5, 0, 0.0);
        bool b2 = false;
        const std::vector<int64_t> without = brute(lone, modes, b2);
        bad = false;
        want = brute(s, modes, bad);
        int kept = 0;
        for (size_t m = 0; m < modes.size() / 3; ++m) kept += std::memcmp(&want[m * W], &without[m * W], 6 * sizeof(int64_t)) != 0;
        check(bad && kept > 0 && kept < (int)(modes.size() / 3), "v_x = 2^40: the term is dropped where |C| = 1 and kept where both products stay below");
        set_velocity(s, 5, 0, 1.0);
    }
    double j[36];
    check(current_read(&st, &err, "g", v, j, nullptr) == LJMD_ERR_RANGE, "read: LJMD_ERR_RANGE");
    check(current_accumulate(&st, &err, "g", v) == LJMD_OK && current_fetch(&st, &err, "g", v, nullptr, nullptr) == LJMD_ERR_RANGE, "sticky");
    check(current_reset(&st, &err, "g", v) == LJMD_OK && current_fetch(&st, &err, "g", v, nullptr, &snaps) == LJMD_OK && snaps == 0, "reset clears the word");
    const int slot = (int)(std::find(s.perm.begin(), s.perm.end(), 9) - s.perm.begin());
    s.pos[(size_t)s.P + slot] = NAN;
    check(current_accumulate(&st, &err, "g", v) == LJMD_OK && current_fetch(&st, &err, "g", v, nullptr, nullptr) == LJMD_ERR_RANGE, "a NaN coordinate sets the word");
    s.pos[(size_t)s.P + slot] = 1.0;
    ResidentView w = v;
    w.L = NAN;
    check(current_reset(&st, &err, "g", v) == LJMD_OK && current_accumulate(&st, &err, "g", w) == LJMD_OK &&
              current_fetch(&st, &err, "g", w, nullptr, nullptr) == LJMD_ERR_RANGE, "L = NaN sets the word");
    current_release(&st, nullptr);
}

// one system in full, for the numpy model: its particles, its modes, the words the core returns
void print_words()
{
    const System s = make_system(65, 2, 7.5, 31);
    const std::vector<int32_t> modes = make_modes(9, 5);
    const ResidentView v = view_of(s);
    CurrentState st;
    std::string err;
    std::vector<int64_t> got(9 * W, -1);
    check(current_configure(&st, &err, "p", v, 9, modes.data(), 1) == LJMD_OK && current_accumulate(&st, &err, "p", v) == LJMD_OK &&
              current_fetch(&st, &err, "p", v, got.data(), nullptr) == LJMD_OK, "the printed system");
    std::printf("L %a\n", s.L);
    for (int i = 0; i < s.n; ++i)
        std::printf("particle %a %a %a %a %a %a\n", s.xyz[3 * (size_t)i], s.xyz[3 * (size_t)i + 1], s.xyz[3 * (size_t)i + 2],
                    s.vxyz[3 * (size_t)i], s.vxyz[3 * (size_t)i + 1], s.vxyz[3 * (size_t)i + 2]);
    for (int m = 0; m < 9; ++m) {
        std::printf("mode %d %d %d\nwords", modes[3 * (size_t)m], modes[3 * (size_t)m + 1], modes[3 * (size_t)m + 2]);
        for (int w = 0; w < W; ++w) std::printf(" %lld", (long long)got[(size_t)m * W + w]);
        std::printf("\n");
    }
    current_release(&st, nullptr);
}

}  // namespace

int main()
{
    setenv("FAKEHIP_DEVICES", "1", 1);
    guards_and_sequences();
    grids_against_brute_force();
    range_flag();
    print_words();
    if (g_failures == 0) std::printf("current_host: ok\n");
    return g_failures == 0 ? 0 : 1;
}
