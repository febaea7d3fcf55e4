// stress_host.cpp -- TEST INFRASTRUCTURE: the host core of the engine's resident pressure tensor (csrc/ljmd_stress.cpp,
// namespace ljmds) without a GPU and without the engine.  Linked from the core, the core of ljmd_rdf.cpp (the walk plan),
// ljmd_common.cpp, the fake HIP runtime (tests/fakehip) and its own definitions of the launchers, which check what they
// are given and carry out on the host what the kernels mean: the tile boxes, the walk with its skipping, tie rule and
// doubling, the per-workgroup partials, the kinetic partials and the fold.  The program checks itself -- every guard with
// its return code and message, the sequences around configure / accumulate / read / reset, a full series, NULL outputs,
// release, the returned words against a brute-force sum over the ordered pairs in particle order, and the plan under a
// grid of LJMD_WALK_CHUNK values (slices, workgroups and partial rows) -- prints one line
// per check that fails and "stress_host: ok" when none did.  tests/test_stress_host.py runs it under ASan and UBSan.
// (The fake hipMalloc cannot fail, so the LJMD_ERR_ALLOC branch of configure is not reached here.)
#include "ljmd.h"
#include "ljmd_internal.h"
#include "ljmd_resident.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <optional>
#include <random>
#include <string>
#include <vector>

using namespace ljmds;
using ljmdk::add192;
using ljmdk::from128;

namespace {

int g_failures = 0;
int g_boxes = 0, g_pairs = 0, g_kinetic = 0, g_fold = 0;
int g_fail_pairs = 0;                      // 1: the next pair launch returns hipErrorLaunchFailure
StressPairArgs g_last{};
dim3 g_grid;
bool g_plan_only = false;                  // the pair launch checks its grid and writes zero rows: no pair is evaluated

void check(bool ok, const char *what)
{
    if (ok) return;
    ++g_failures;
    std::printf("FAILED: %s\n", what);
}

bool has(const std::string &err, const char *text) { return err.find(text) != std::string::npos; }

// Q(t) = RNE(t 2^64) for |t| < 2^40, the splitting of ljmd_internal.h's fixed_add
__int128 Q(double t)
{
    const double v = std::nearbyint(t * 0x1p64);
    const double hi = std::trunc(v * 0x1p-62);
    const double lo = v - hi * 0x1p62;
    return (__int128)(int64_t)hi * ((__int128)1 << 62) + (__int128)(int64_t)lo;
}

bool out_of_range(double t) { return !(std::fabs(t) < 0x1p40); }

// acc[c] += Q(t[c]), or six zeros and the flag
void add_six(__int128 (&acc)[6], const double (&t)[6], bool oob, bool &bad)
{
    for (double x : t) oob = oob || out_of_range(x);
    bad = bad || oob;
    for (int c = 0; c < 6; ++c) acc[c] += oob ? 0 : Q(t[c]);
}

// the definition's pair (i, j): six terms into acc; false when r2 >= rc2
void pair_terms(const double *pi, const double *pj, double L, double invL, double rc2, __int128 (&acc)[6], bool &bad)
{
    double d[3];
    for (int k = 0; k < 3; ++k) {
        const double d0 = pi[k] - pj[k];
        d[k] = d0 - L * std::round(d0 * invL);
    }
    const double r2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
    if (!(r2 < rc2)) return;
    const double u = 1.0 / r2, u3 = u * u * u, u6 = u3 * u3, mdu = 2.0 * u6 - u3;
    const double fx = mdu * d[0] * u, fy = mdu * d[1] * u, fz = mdu * d[2] * u;
    const double t[6] = {fx * d[0], fy * d[1], fz * d[2], fx * d[1], fx * d[2], fy * d[2]};
    add_six(acc, t, out_of_range(fx) || out_of_range(fy) || out_of_range(fz) || out_of_range(u6), bad);
}

void add128(uint64_t (&q)[3], __int128 x)
{
    uint64_t o[3];
    from128(o, x);
    add192(q, o);
}

}  // namespace

namespace ljmdr {

hipError_t launch_rdf_boxes(const RdfBoxArgs &a, hipStream_t)
{
    ++g_boxes;
    check(a.pos && a.bbox && a.T >= 1 && a.TB >= 1 && a.T % a.TB == 0, "box launch: arguments");
    for (int t = 0; t < a.T; ++t) {
        const int g = t / a.TB, tl = t - g * a.TB;
        double *o = a.bbox + (size_t)t * kRdfBoxStride;
        for (int k = 0; k < 3; ++k) { o[k] = INFINITY; o[3 + k] = -INFINITY; }
        for (int l = 0; l < 64; ++l)
            for (int k = 0; k < 3; ++k) {
                const double x = a.pos[((size_t)g * 3 + k) * a.P + (size_t)tl * 64 + l];
                if (x == x) { o[k] = std::fmin(o[k], x); o[3 + k] = std::fmax(o[3 + k], x); }
            }
    }
    return hipSuccess;
}

hipError_t launch_rdf_pairs(const RdfPairArgs &, dim3, hipStream_t) { return hipErrorLaunchFailure; }   // never called

}  // namespace ljmdr

namespace ljmds {

// stress_pairs_kernel on the host: the same walk, workgroup by workgroup, wave by wave, lane by lane
hipError_t launch_stress_pairs(const StressPairArgs &a, dim3 grid, hipStream_t)
{
    ++g_pairs;
    if (g_fail_pairs > 0 && --g_fail_pairs == 0) return hipErrorLaunchFailure;
    g_last = a;
    check(a.T == a.G * a.TB && a.rank >= 0 && a.rank < a.G, "pair launch: tiles and rank");
    check(a.U == (a.G == 1 ? a.T / 2 + 1 : a.T), "pair launch: steps of the walk");
    check(a.chunk >= 1 && (long long)grid.y * a.chunk >= a.U && (long long)(grid.y - 1) * a.chunk < a.U,
          "pair launch: the slices cover the walk, none is empty");
    check((long long)grid.x * kRdfWaves >= a.TB && (long long)(grid.x - 1) * kRdfWaves < a.TB, "pair launch: row blocks");
    check(a.rc2_skin > a.rc2 && a.rc2_skin < a.rc2 * (1.0 + 1e-9), "pair launch: rc^2 < skip bound");
    g_grid = grid;
    if (g_plan_only) {                                       // every workgroup's rows exist (ASan) and are written
        for (size_t wg = 0; wg < (size_t)grid.x * grid.y; ++wg) {
            std::memset(a.part + wg * 18, 0, 18 * sizeof(uint64_t));
            a.pcount[2 * wg] = 1;
            a.pcount[2 * wg + 1] = 2;
            a.pflag[wg] = 0u;
        }
        return hipSuccess;
    }
    const bool unordered = a.G == 1;
    const int half = (unordered && (a.T & 1) == 0) ? a.T / 2 : -1;
    for (unsigned by = 0; by < grid.y; ++by)
        for (unsigned bx = 0; bx < grid.x; ++bx) {
            const size_t wg = (size_t)by * grid.x + bx;
            uint64_t part[6][3] = {};
            unsigned long long vis = 0, con = 0;
            bool bad = false;
            for (int wave = 0; wave < kRdfWaves; ++wave) {
                const int Il = (int)bx * kRdfWaves + wave;
                if (Il >= a.TB) continue;
                const int I = a.rank * a.TB + Il;
                const double *bi = a.bbox + (size_t)I * kRdfBoxStride;
                const int u0 = (int)by * a.chunk, u1 = std::min(u0 + a.chunk, a.U);
                for (int u = u0; u < u1; ++u) {
                    int J = unordered ? I + u : u;
                    if (J >= a.T) J -= a.T;
                    if (u == half && I >= half) continue;
                    ++con;
                    if (a.skip && J != I && ljmdr::rdf_tile_gap2(bi, a.bbox + (size_t)J * kRdfBoxStride, a.L) > a.rc2_skin) continue;
                    ++vis;
                    const int gj = J / a.TB, jl = J - gj * a.TB;
                    for (int lane = 0; lane < 64; ++lane) {
                        __int128 acc[6] = {};
                        double pi[3], pj[3];
                        for (int k = 0; k < 3; ++k) pi[k] = a.pos[((size_t)a.rank * 3 + k) * a.P + (size_t)Il * 64 + lane];
                        for (int j = 0; j < 64; ++j) {
                            if (J == I && (unordered ? j <= lane : j == lane)) continue;
                            for (int k = 0; k < 3; ++k) pj[k] = a.pos[((size_t)gj * 3 + k) * a.P + (size_t)jl * 64 + j];
                            pair_terms(pi, pj, a.L, a.invL, a.rc2, acc, bad);
                        }
                        for (int c = 0; c < 6; ++c) {
                            add128(part[c], acc[c]);
                            if (unordered) add128(part[c], acc[c]);
                        }
                    }
                }
            }
            std::memcpy(a.part + wg * 18, part, sizeof part);
            a.pcount[2 * wg] = vis;
            a.pcount[2 * wg + 1] = con;
            a.pflag[wg] = bad ? 1u : 0u;
        }
    return hipSuccess;
}

hipError_t launch_stress_kinetic(const StressKineticArgs &a, hipStream_t)
{
    ++g_kinetic;
    check(a.v && a.kpart && a.kflag && a.blocks == (a.P + kStressKinBlock - 1) / kStressKinBlock, "kinetic launch: arguments");
    for (int b = 0; b < a.blocks; ++b) {
        uint64_t part[6][3] = {};
        bool bad = false;
        for (size_t s = (size_t)b * kStressKinBlock; s < std::min((size_t)a.P, (size_t)(b + 1) * kStressKinBlock); ++s) {
            const double vx = a.v[s], vy = a.v[a.P + s], vz = a.v[2 * (size_t)a.P + s];
            const double t[6] = {vx * vx, vy * vy, vz * vz, vx * vy, vx * vz, vy * vz};
            __int128 acc[6] = {};
            add_six(acc, t, false, bad);
            for (int c = 0; c < 6; ++c) add128(part[c], acc[c]);
        }
        std::memcpy(a.kpart + (size_t)b * 18, part, sizeof part);
        a.kflag[b] = bad ? 1u : 0u;
    }
    return hipSuccess;
}

hipError_t launch_stress_fold(const StressFoldArgs &a, hipStream_t)
{
    ++g_fold;
    check(a.part && a.kpart && a.row && a.count && a.range && a.workgroups >= 1 && a.blocks >= 1, "fold launch: arguments");
    uint64_t row[12][3] = {};
    unsigned long long c0 = 0, c1 = 0;
    bool bad = false;
    for (int b = 0; b < a.blocks; ++b) {
        for (int c = 0; c < 6; ++c) {
            const uint64_t *p = a.kpart + ((size_t)b * 6 + c) * 3;
            const uint64_t o[3] = {p[0], p[1], p[2]};
            add192(row[c], o);
        }
        bad = bad || a.kflag[b];
    }
    for (int w = 0; w < a.workgroups; ++w) {
        for (int c = 0; c < 6; ++c) {
            const uint64_t *p = a.part + ((size_t)w * 6 + c) * 3;
            const uint64_t o[3] = {p[0], p[1], p[2]};
            add192(row[6 + c], o);
        }
        bad = bad || a.pflag[w];
        c0 += a.pcount[2 * (size_t)w];
        c1 += a.pcount[2 * (size_t)w + 1];
    }
    std::memcpy(a.row, row, sizeof row);
    a.count[0] = c0;
    a.count[1] = c1;
    if (bad) *a.range = 1;
    return hipSuccess;
}

}  // namespace ljmds

namespace {

// a system in the engine's layout: G blocks of TB tiles, S live particles per block, NaN / 0 on the padding
struct System {
    int n, G, S, TB, P;
    double L, rc;
    std::vector<double> pos, vel;      // [G][3][P] each (a rank's own velocities are block `rank` of vel)
    std::vector<double> xyz, v;        // [n][3] in particle order, for the brute force
};

System make_system(int n, int G, int TB, double L, double rc, unsigned seed)
{
    System s;
    s.n = n; s.G = G; s.S = n / G; s.TB = TB; s.P = TB * 64; s.L = L; s.rc = rc;
    s.pos.assign((size_t)G * 3 * s.P, NAN);
    s.vel.assign((size_t)G * 3 * s.P, 0.0);
    std::mt19937_64 rng(seed);
    std::uniform_real_distribution<double> u(0.0, 1.0);
    for (int i = 0; i < n; ++i) {
        const int g = i / s.S, l = i - g * s.S;
        // a jittered simple-cubic lattice of spacing L / 10, filled layer by layer: no pair closer than 0.6 L / 10, and a
        // tile is a thin slab, so that the walk does skip
        const int site[3] = {i % 10, i / 10 % 10, i / 100};
        for (int k = 0; k < 3; ++k) {
            const double x = (site[k] + 0.3 + 0.4 * u(rng)) * 0.1 * L;
            const double w = 2.0 * u(rng) - 1.0;
            s.pos[((size_t)g * 3 + k) * s.P + l] = x;
            s.vel[((size_t)g * 3 + k) * s.P + l] = w;
            s.xyz.push_back(x);
            s.v.push_back(w);
        }
    }
    return s;
}

ResidentView view_of(const System &s, int rank, bool compact = true)
{
    ResidentView v;
    v.n = s.n; v.P = s.P; v.TB = s.TB; v.T = s.G * s.TB; v.G = s.G; v.rank = rank;
    v.L = s.L; v.invL = 1.0 / s.L; v.rc2 = s.rc * s.rc;
    v.pos = s.pos.data();
    v.v = s.vel.data() + (size_t)rank * 3 * s.P;
    v.stream = nullptr;
    v.compact = compact;
    return v;
}

// K and S of the definition over the ordered pairs (i in [i0, i1), j != i), in particle order
void brute(const System &s, int i0, int i1, uint64_t (&row)[12][3], bool &bad)
{
    std::memset(row, 0, sizeof row);
    for (int i = i0; i < i1; ++i) {
        const double *w = &s.v[3 * (size_t)i];
        const double t[6] = {w[0] * w[0], w[1] * w[1], w[2] * w[2], w[0] * w[1], w[0] * w[2], w[1] * w[2]};
        __int128 k[6] = {}, acc[6] = {};
        add_six(k, t, false, bad);
        for (int j = 0; j < s.n; ++j)
            if (j != i) pair_terms(&s.xyz[3 * (size_t)i], &s.xyz[3 * (size_t)j], s.L, 1.0 / s.L, s.rc * s.rc, acc, bad);
        for (int c = 0; c < 6; ++c) {
            add128(row[c], k[c]);
            add128(row[6 + c], acc[c]);
        }
    }
}

void guards_and_sequences()
{
    const System s = make_system(300, 1, 8, 10.0, 2.5, 1);
    const ResidentView v = view_of(s, 0);
    StressState st;
    std::string err;
    std::vector<int64_t> words(4 * kStressWords, -1);
    std::vector<double> p(4 * 6, -1.0);
    int64_t snaps = -1, vis = -1, tot = -1;
    double ms = -1.0;
    const char *who = "caller";

    // before configure
    check(stress_accumulate(&st, &err, who, v) == LJMD_ERR_STATE && has(err, "caller: the pressure tensor is not configured"),
          "accumulate before configure");
    check(stress_fetch(&st, &err, who, v, words.data(), &snaps) == LJMD_ERR_STATE && has(err, "not configured"), "read_exact before configure");
    check(stress_read(&st, &err, who, v, p.data(), &snaps) == LJMD_ERR_STATE && has(err, "not configured"), "read before configure");
    check(stress_reset(&st, &err, who, v) == LJMD_ERR_STATE && has(err, "not configured"), "reset before configure");
    check(stress_profile_read(&st, &err, who, v, &vis, &tot, &ms) == LJMD_ERR_STATE, "profile_read before configure");
    check(g_boxes + g_pairs + g_kinetic + g_fold == 0, "nothing launched before configure");
    stress_release(&st, nullptr);                            // what ljmd_destroy does on a handle never configured

    // guards of configure, each leaving what was there
    check(stress_configure(&st, &err, who, v, -1) == LJMD_ERR_INVALID_ARG && has(err, "caller: max_snapshots = -1 outside 1..262144"),
          "max_snapshots < 0");
    check(stress_configure(&st, &err, who, v, kStressMaxSnapshots + 1) == LJMD_ERR_INVALID_ARG && has(err, "max_snapshots = 262145"),
          "max_snapshots too large");
    ResidentView big = v;
    big.n = kStressMaxN + 1;
    check(stress_configure(&st, &err, who, big, 4) == LJMD_ERR_INVALID_ARG && has(err, "caller: n = 8388609 outside 1..8388608"), "n too large");
    check(st.max_snapshots == 0 && !st.d_series && !st.d_part && !st.d_bbox, "refused configure allocates nothing");
    check(stress_configure(&st, &err, who, big, 0) == LJMD_OK, "off needs no valid n");

    check(stress_configure(&st, &err, who, v, 3) == LJMD_OK && st.max_snapshots == 3 && st.d_series && st.d_part && st.d_kpart &&
              st.d_bbox && st.d_range && st.workgroups >= 1 && st.blocks == 1, "configure");
    check(stress_configure(&st, &err, who, v, -5) == LJMD_ERR_INVALID_ARG && st.max_snapshots == 3, "a refused reconfigure keeps the configuration");
    check(stress_fetch(&st, &err, who, v, words.data(), &snaps) == LJMD_OK && snaps == 0 && words[0] == -1, "an empty series copies nothing");
    check(stress_profile_read(&st, &err, who, v, &vis, &tot, &ms) == LJMD_OK && vis == 0 && tot == 0 && ms == 0.0,
          "profile before the first accumulate");

    // the words against brute force
    uint64_t want[12][3];
    bool bad = false;
    brute(s, 0, s.n, want, bad);
    check(!bad, "the test system is in range");
    check(stress_accumulate(&st, &err, who, v) == LJMD_OK && g_boxes == 1 && g_pairs == 1 && g_kinetic == 1 && g_fold == 1,
          "accumulate: four launches");
    check(g_last.skip == 1 && g_last.G == 1 && g_last.pos == v.pos && g_last.bbox == st.d_bbox && g_last.L == 10.0 &&
              g_last.rc2 == 6.25, "accumulate: arguments");
    check(stress_fetch(&st, &err, who, v, words.data(), &snaps) == LJMD_OK && snaps == 1 &&
              std::memcmp(words.data(), want, sizeof want) == 0, "one snapshot equals the brute-force sum");
    check(words[kStressWords] == -1, "read_exact writes the taken snapshots only");
    check(stress_profile_read(&st, &err, who, v, &vis, &tot, &ms) == LJMD_OK && tot == 8 * 4 + 4 && vis > 0 && vis < tot,
          "profile: T (T / 2) + T / 2 tile pairs considered, some skipped");
    check(stress_profile_read(&st, &err, who, v, nullptr, nullptr, nullptr) == LJMD_OK, "profile with NULL pointers");
    check(stress_fetch(&st, &err, who, v, nullptr, nullptr) == LJMD_OK && stress_read(&st, &err, who, v, nullptr, nullptr) == LJMD_OK,
          "reads with NULL pointers");

    // doubles: ljmd_stress_from_exact on the same words
    double p1[6];
    check(stress_read(&st, &err, who, v, p.data(), &snaps) == LJMD_OK && snaps == 1 && p[6] == -1.0, "read");
    check(ljmd_stress_from_exact(words.data(), 10.0, p1) == LJMD_OK && std::memcmp(p1, p.data(), sizeof p1) == 0,
          "read = ljmd_stress_from_exact of read_exact");
    check(p[0] > 0.0 && std::isfinite(p[3]), "a kinetic diagonal is positive");
    check(ljmd_stress_from_exact(nullptr, 10.0, p1) == LJMD_ERR_INVALID_ARG && ljmd_stress_from_exact(words.data(), 10.0, nullptr) == LJMD_ERR_INVALID_ARG &&
              ljmd_stress_from_exact(words.data(), 0.0, p1) == LJMD_ERR_INVALID_ARG && ljmd_stress_from_exact(words.data(), NAN, p1) == LJMD_ERR_INVALID_ARG,
          "ljmd_stress_from_exact: guards");

    // not compact: nothing may be skipped, the same words
    check(stress_accumulate(&st, &err, who, view_of(s, 0, false)) == LJMD_OK && g_last.skip == 0, "positions not compact: skip off");
    check(stress_profile_read(&st, &err, who, v, &vis, &tot, &ms) == LJMD_OK && vis == tot, "not compact: visited = total");
    check(stress_fetch(&st, &err, who, v, words.data(), &snaps) == LJMD_OK && snaps == 2 &&
              std::memcmp(words.data() + kStressWords, want, sizeof want) == 0, "the second row equals the first");

    // a failed launch: reported, not counted
    g_fail_pairs = 1;
    check(stress_accumulate(&st, &err, who, v) == LJMD_ERR_HIP && has(err, "caller: pressure tensor launch failed"), "failed launch");
    check(stress_fetch(&st, &err, who, v, nullptr, &snaps) == LJMD_OK && snaps == 2, "failed launch adds no snapshot");

    // a full series
    check(stress_accumulate(&st, &err, who, v) == LJMD_OK, "third snapshot");
    const int launches = g_boxes + g_pairs + g_kinetic + g_fold;
    check(stress_accumulate(&st, &err, who, v) == LJMD_ERR_STATE && has(err, "caller: the series is full (3 snapshots"), "full series");
    check(g_boxes + g_pairs + g_kinetic + g_fold == launches, "a full series launches nothing");
    check(stress_fetch(&st, &err, who, v, words.data(), &snaps) == LJMD_OK && snaps == 3, "full series reads");
    check(stress_reset(&st, &err, who, v) == LJMD_OK && stress_fetch(&st, &err, who, v, nullptr, &snaps) == LJMD_OK && snaps == 0, "reset empties");
    check(stress_accumulate(&st, &err, who, v) == LJMD_OK, "room again after reset");

    // an engine of another shape
    const System other = make_system(600, 1, 12, 10.0, 2.5, 2);
    check(stress_accumulate(&st, &err, who, view_of(other, 0)) == LJMD_ERR_STATE && has(err, "not the one the pressure tensor was configured for"),
          "a view of another shape is refused");

    // reconfigure empties, off frees
    check(stress_configure(&st, &err, who, v, 2) == LJMD_OK && st.max_snapshots == 2 && st.snapshots == 0, "reconfigure");
    check(stress_configure(&st, &err, who, v, 0) == LJMD_OK && st.max_snapshots == 0 && !st.d_series && !st.d_part && !st.d_kpart &&
              !st.d_bbox && !st.timer.ev0 && !st.timer.ev1, "off frees");
    check(stress_accumulate(&st, &err, who, v) == LJMD_ERR_STATE && stress_fetch(&st, &err, who, v, nullptr, nullptr) == LJMD_ERR_STATE,
          "off: as before configure");
    check(stress_configure(&st, &err, who, v, 2) == LJMD_OK && stress_accumulate(&st, &err, who, v) == LJMD_OK, "configured again");
    stress_release(&st, nullptr);                            // what ljmd_destroy does on a configured handle
    check(st.max_snapshots == 0 && !st.d_series, "release");
    stress_release(&st, nullptr);
}

// odd and even tile counts, one slice and many, wide boxes: always the brute-force integers
void walks_against_brute_force()
{
    struct Case { int n, TB; double rc; };
    const Case cases[] = {{200, 5, 2.5}, {256, 4, 4.9}, {130, 3, 1.2}, {64, 1, 4.9}, {2, 1, 4.9}};
    for (const Case &c : cases) {
        const System s = make_system(c.n, 1, c.TB, 10.0, c.rc, 100 + c.n);
        const ResidentView v = view_of(s, 0);
        StressState st;
        std::string err;
        uint64_t want[12][3];
        int64_t got[kStressWords];
        bool bad = false;
        brute(s, 0, s.n, want, bad);
        check(stress_configure(&st, &err, "w", v, 1) == LJMD_OK && stress_accumulate(&st, &err, "w", v) == LJMD_OK &&
                  stress_fetch(&st, &err, "w", v, got, nullptr) == LJMD_OK && std::memcmp(got, want, sizeof want) == 0,
              "one-rank walk equals the brute-force sum");
        check(!bad, "walk cases are in range");
        stress_release(&st, nullptr);
    }
}

// LJMD_WALK_CHUNK: configure sizes the partial rows from the plan accumulate launches from, for every override of the grid
// tests/rdf_host enumerates; the launcher's own checks (the slices cover the walk, none is empty) run on each
void plans_under_an_override()
{
    const int TBs[] = {1, 4, 5, 33, 36, 64, 65, 132, 260};
    const int Gs[] = {1, 2, 3, 4, 8};
    g_plan_only = true;
    for (int TB : TBs)
        for (int G : Gs) {
            const int T = G * TB, U = G == 1 ? T / 2 + 1 : T, P = TB * 64;
            const std::vector<double> pos((size_t)G * 3 * P, NAN), vel((size_t)3 * P, 0.0);
            const int asked[] = {1, 2, 63, 64, 65, U - 1, U, U + 7};
            for (int chunk : asked) {
                ResidentView v;
                v.n = T * 64; v.P = P; v.TB = TB; v.T = T; v.G = G; v.rank = G - 1;
                v.L = 10.0; v.invL = 0.1; v.rc2 = 6.25;
                v.pos = pos.data();
                v.v = vel.data();
                v.compact = true;
                v.walk_chunk = chunk;
                const int want_chunk = std::max(1, std::min(chunk, U));
                const int slices = (U + want_chunk - 1) / want_chunk, row_blocks = (TB + kRdfWaves - 1) / kRdfWaves;
                StressState st;
                std::string err;
                int64_t vis = -1, tot = -1;
                check(stress_configure(&st, &err, "o", v, 1) == LJMD_OK && st.workgroups == row_blocks * slices,
                      "override: configure sizes the partial rows from the overridden plan");
                check(stress_accumulate(&st, &err, "o", v) == LJMD_OK && g_last.chunk == want_chunk && g_last.U == U &&
                          (int)g_grid.x == row_blocks && (int)g_grid.y == slices && (int)(g_grid.x * g_grid.y) == st.workgroups,
                      "override: accumulate launches the plan configure sized for");
                check(stress_profile_read(&st, &err, "o", v, &vis, &tot, nullptr) == LJMD_OK && vis == st.workgroups &&
                          tot == 2 * (int64_t)st.workgroups, "override: the fold reads one row per workgroup");
                // a view with another value of the knob is another plan: refused, unless the grid happens to be the same
                ResidentView other = v;
                other.walk_chunk = std::nullopt;
                const ljmdr::RdfWalk w = ljmdr::rdf_plan_walk(TB, T, G, std::nullopt);
                StressState st2;
                check(stress_configure(&st2, &err, "o", other, 2) == LJMD_OK, "override: configure without the knob");
                check((stress_accumulate(&st2, &err, "o", v) == LJMD_OK) == (w.row_blocks * w.slices == st.workgroups),
                      "override: a view whose plan needs other partial rows is refused");
                stress_release(&st, nullptr);
                stress_release(&st2, nullptr);
            }
        }
    g_plan_only = false;
}

// rank engines: own rows x all columns; the partials add up to the one-rank words as integers
void rank_partials()
{
    const int G = 3;
    const System s = make_system(390, G, 4, 10.0, 3.0, 7);
    uint64_t all[12][3], sum[12][3] = {};
    bool bad = false;
    brute(s, 0, s.n, all, bad);
    for (int g = 0; g < G; ++g) {
        const ResidentView v = view_of(s, g);
        StressState st;
        std::string err;
        uint64_t want[12][3];
        int64_t got[kStressWords];
        brute(s, g * s.S, (g + 1) * s.S, want, bad);
        check(stress_configure(&st, &err, "r", v, 1) == LJMD_OK && stress_accumulate(&st, &err, "r", v) == LJMD_OK &&
                  g_last.G == G && g_last.rank == g && g_last.U == v.T, "rank view: arguments");
        check(stress_fetch(&st, &err, "r", v, got, nullptr) == LJMD_OK && std::memcmp(got, want, sizeof want) == 0,
              "a rank's partial equals its rows of the brute-force sum");
        for (int c = 0; c < 12; ++c) {
            const uint64_t o[3] = {(uint64_t)got[3 * c], (uint64_t)got[3 * c + 1], (uint64_t)got[3 * c + 2]};
            add192(sum[c], o);
        }
        stress_release(&st, nullptr);
    }
    check(std::memcmp(sum, all, sizeof all) == 0 && !bad, "the rank partials add up to the definition");
}

// a pair 0.05 apart: its terms enter as 0, the sticky word is set until reset, nothing else is disturbed
void range_flag()
{
    System s = make_system(128, 1, 2, 10.0, 2.5, 9);
    for (int k = 0; k < 3; ++k) s.pos[(size_t)k * s.P + 1] = s.pos[(size_t)k * s.P] + (k == 0 ? 0.05 : 0.0);
    for (int k = 0; k < 3; ++k) s.xyz[3 + k] = s.pos[(size_t)k * s.P + 1];
    const ResidentView v = view_of(s, 0);
    StressState st;
    std::string err;
    uint64_t want[12][3];
    int64_t got[kStressWords];
    int64_t snaps = -1;
    bool bad = false;
    brute(s, 0, s.n, want, bad);
    check(bad, "0.05 apart is out of range");
    check(stress_configure(&st, &err, "g", v, 4) == LJMD_OK && stress_accumulate(&st, &err, "g", v) == LJMD_OK, "accumulate succeeds");
    check(stress_fetch(&st, &err, "g", v, got, &snaps) == LJMD_ERR_RANGE && has(err, "g: a pair's or a particle's") &&
              has(err, "until ljmd_stress_reset") && snaps == -1, "read_exact: LJMD_ERR_RANGE");
    check(std::memcmp(got, want, sizeof want) == 0, "the flagged pair entered as zeros, everything else as usual");
    double p[6];
    check(stress_read(&st, &err, "g", v, p, nullptr) == LJMD_ERR_RANGE, "read: LJMD_ERR_RANGE");
    check(stress_accumulate(&st, &err, "g", v) == LJMD_OK && stress_fetch(&st, &err, "g", v, nullptr, nullptr) == LJMD_ERR_RANGE, "sticky");
    check(stress_reset(&st, &err, "g", v) == LJMD_OK && stress_fetch(&st, &err, "g", v, nullptr, &snaps) == LJMD_OK && snaps == 0,
          "reset clears the word");
    // a velocity product out of range
    s.vel[5] = 0x1p21;
    s.pos[1] = NAN;                                          // the close pair is gone: slot 1 fails every cutoff test now
    check(stress_accumulate(&st, &err, "g", v) == LJMD_OK && stress_fetch(&st, &err, "g", v, got, nullptr) == LJMD_ERR_RANGE,
          "a velocity product of 2^42 sets the word");
    stress_release(&st, nullptr);
}

}  // namespace

int main()
{
    setenv("FAKEHIP_DEVICES", "1", 1);
    guards_and_sequences();
    walks_against_brute_force();
    rank_partials();
    plans_under_an_override();
    range_flag();
    if (g_failures == 0) std::printf("stress_host: ok\n");
    return g_failures == 0 ? 0 : 1;
}
