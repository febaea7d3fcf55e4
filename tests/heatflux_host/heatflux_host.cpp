// heatflux_host.cpp -- TEST INFRASTRUCTURE: the host core of the engine's resident heat flux (csrc/ljmd_heatflux.cpp,
// namespace ljmdq) without a GPU and without the engine.  Linked from the core, the core of ljmd_rdf.cpp (the walk plan),
// ljmd_common.cpp, the fake HIP runtime (tests/fakehip) and its own definitions of the launchers, which check what they
// are given and carry out on the host what the kernels mean: the tile boxes, the unordered walk with its skipping, tie
// rule and doubling, the per-workgroup partials, the convective partials and the fold.  The program checks itself --
// every guard with its return code and message in order, the refusal of rank engines and multi-device views, the
// sequences around configure / accumulate / read / reset, a full series, NULL outputs, release, the range word, and the
// returned words against a brute-force sum over the ordered pairs in particle order -- prints one line per check that
// fails and "heatflux_host: ok" when none did.  tests/test_heatflux_host.py runs it under ASan and UBSan.
// (The fake hipMalloc cannot fail, so the LJMD_ERR_ALLOC branch of configure is not reached here.)
#include "ljmd.h"
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

using namespace ljmdq;
using ljmdk::add192;
using ljmdk::from128;

namespace {

int g_failures = 0;
int g_boxes = 0, g_pairs = 0, g_kinetic = 0, g_fold = 0;
int g_fail_pairs = 0;                      // 1: the next pair launch returns hipErrorLaunchFailure
HeatfluxPairArgs g_last{};
dim3 g_grid;

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

// the definition's pair (i, j): six terms into acc; nothing when r2 >= rc2
void pair_terms(const double *pi, const double *pj, const double *vi, const double *vj, double L, double invL, double rc2,
                __int128 (&acc)[6], bool &bad)
{
    double d[3], w[3];
    for (int k = 0; k < 3; ++k) {
        const double d0 = pi[k] - pj[k];
        d[k] = d0 - L * std::round(d0 * invL);
        w[k] = vi[k] + vj[k];
    }
    const double r2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
    if (!(r2 < rc2)) return;
    const double u = 1.0 / r2, u3 = u * u * u, u6 = u3 * u3, mdu = 2.0 * u6 - u3;
    const double fx = mdu * d[0] * u, fy = mdu * d[1] * u, fz = mdu * d[2] * u;
    const double phi = u6 - u3;
    const double g = fx * w[0] + fy * w[1] + fz * w[2];
    const double t[6] = {phi * w[0], phi * w[1], phi * w[2], g * d[0], g * d[1], g * d[2]};
    bool oob = out_of_range(fx) || out_of_range(fy) || out_of_range(fz) || out_of_range(u6) || out_of_range(w[0]) ||
               out_of_range(w[1]) || out_of_range(w[2]) || out_of_range(g);
    for (double x : t) oob = oob || out_of_range(x);
    bad = bad || oob;
    for (int c = 0; c < 6; ++c) acc[c] += oob ? 0 : Q(t[c]);
}

// the definition's particle: three terms into acc
void kinetic_terms(double vx, double vy, double vz, __int128 (&acc)[3], bool &bad)
{
    const double k2 = vx * vx + vy * vy + vz * vz;
    const double t[3] = {k2 * vx, k2 * vy, k2 * vz};
    bool oob = out_of_range(k2);
    for (double x : t) oob = oob || out_of_range(x);
    bad = bad || oob;
    for (int c = 0; c < 3; ++c) acc[c] += oob ? 0 : Q(t[c]);
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

namespace ljmdq {

// heatflux_pairs_kernel on the host: the same walk, workgroup by workgroup, wave by wave, lane by lane
hipError_t launch_heatflux_pairs(const HeatfluxPairArgs &a, dim3 grid, hipStream_t)
{
    ++g_pairs;
    if (g_fail_pairs > 0 && --g_fail_pairs == 0) return hipErrorLaunchFailure;
    g_last = a;
    check(a.pos && a.vel && a.bbox && a.T >= 1 && (long long)a.P >= (long long)a.T * 64, "pair launch: arguments");
    check(a.U == a.T / 2 + 1, "pair launch: steps of the unordered walk");
    check(a.chunk >= 1 && (long long)grid.y * a.chunk >= a.U && (long long)(grid.y - 1) * a.chunk < a.U,
          "pair launch: the slices cover the walk, none is empty");
    check((long long)grid.x * kRdfWaves >= a.T && (long long)(grid.x - 1) * kRdfWaves < a.T, "pair launch: row blocks");
    check(a.rc2_skin > a.rc2 && a.rc2_skin < a.rc2 * (1.0 + 1e-9), "pair launch: rc^2 < skip bound");
    g_grid = grid;
    const int half = (a.T & 1) == 0 ? a.T / 2 : -1;
    const size_t P = (size_t)a.P;
    for (unsigned by = 0; by < grid.y; ++by)
        for (unsigned bx = 0; bx < grid.x; ++bx) {
            const size_t wg = (size_t)by * grid.x + bx;
            uint64_t part[6][3] = {};
            unsigned long long vis = 0, con = 0;
            bool bad = false;
            for (int wave = 0; wave < kRdfWaves; ++wave) {
                const int I = (int)bx * kRdfWaves + wave;
                if (I >= a.T) continue;
                const double *bi = a.bbox + (size_t)I * kRdfBoxStride;
                const int u0 = (int)by * a.chunk, u1 = std::min(u0 + a.chunk, a.U);
                for (int u = u0; u < u1; ++u) {
                    int J = I + u;
                    if (J >= a.T) J -= a.T;
                    if (u == half && I >= half) continue;
                    ++con;
                    if (a.skip && J != I && ljmdr::rdf_tile_gap2(bi, a.bbox + (size_t)J * kRdfBoxStride, a.L) > a.rc2_skin) continue;
                    ++vis;
                    for (int lane = 0; lane < 64; ++lane) {
                        __int128 acc[6] = {};
                        double pi[3], pj[3], vi[3], vj[3];
                        for (int k = 0; k < 3; ++k) {
                            pi[k] = a.pos[k * P + (size_t)I * 64 + lane];
                            vi[k] = a.vel[k * P + (size_t)I * 64 + lane];
                        }
                        for (int j = 0; j < 64; ++j) {
                            if (J == I && j <= lane) continue;
                            for (int k = 0; k < 3; ++k) {
                                pj[k] = a.pos[k * P + (size_t)J * 64 + j];
                                vj[k] = a.vel[k * P + (size_t)J * 64 + j];
                            }
                            pair_terms(pi, pj, vi, vj, a.L, a.invL, a.rc2, acc, bad);
                        }
                        for (int c = 0; c < 6; ++c) {
                            add128(part[c], acc[c]);
                            add128(part[c], acc[c]);                // both orders of every pair
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

hipError_t launch_heatflux_kinetic(const HeatfluxKineticArgs &a, hipStream_t)
{
    ++g_kinetic;
    check(a.v && a.kpart && a.kflag && a.blocks == (a.P + kHeatfluxKinBlock - 1) / kHeatfluxKinBlock, "kinetic launch: arguments");
    for (int b = 0; b < a.blocks; ++b) {
        uint64_t part[3][3] = {};
        bool bad = false;
        for (size_t s = (size_t)b * kHeatfluxKinBlock; s < std::min((size_t)a.P, (size_t)(b + 1) * kHeatfluxKinBlock); ++s) {
            __int128 acc[3] = {};
            kinetic_terms(a.v[s], a.v[a.P + s], a.v[2 * (size_t)a.P + s], acc, bad);
            for (int c = 0; c < 3; ++c) add128(part[c], acc[c]);
        }
        std::memcpy(a.kpart + (size_t)b * 9, part, sizeof part);
        a.kflag[b] = bad ? 1u : 0u;
    }
    return hipSuccess;
}

hipError_t launch_heatflux_fold(const HeatfluxFoldArgs &a, hipStream_t)
{
    ++g_fold;
    check(a.part && a.kpart && a.row && a.count && a.range && a.workgroups >= 1 && a.blocks >= 1, "fold launch: arguments");
    uint64_t row[9][3] = {};
    unsigned long long c0 = 0, c1 = 0;
    bool bad = false;
    for (int b = 0; b < a.blocks; ++b) {
        for (int c = 0; c < 3; ++c) {
            const uint64_t *p = a.kpart + ((size_t)b * 3 + c) * 3;
            const uint64_t o[3] = {p[0], p[1], p[2]};
            add192(row[c], o);
        }
        bad = bad || a.kflag[b];
    }
    for (int w = 0; w < a.workgroups; ++w) {
        for (int c = 0; c < 6; ++c) {
            const uint64_t *p = a.part + ((size_t)w * 6 + c) * 3;
            const uint64_t o[3] = {p[0], p[1], p[2]};
            add192(row[3 + c], o);
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

}  // namespace ljmdq

namespace {

// a one-rank system in the engine's layout: T tiles, n live particles, NaN / 0 on the padding
struct System {
    int n, T, P;
    double L, rc;
    std::vector<double> pos, vel;      // [3][P] each
    std::vector<double> xyz, v;        // [n][3] in particle order, for the brute force
};

System make_system(int n, int T, double L, double rc, unsigned seed)
{
    System s;
    s.n = n; s.T = T; s.P = T * 64; s.L = L; s.rc = rc;
    s.pos.assign((size_t)3 * s.P, NAN);
    s.vel.assign((size_t)3 * s.P, 0.0);
    std::mt19937_64 rng(seed);
    std::uniform_real_distribution<double> u(0.0, 1.0);
    for (int i = 0; i < n; ++i) {
        // a jittered simple-cubic lattice of spacing L / 10, filled layer by layer: no pair closer than 0.6 L / 10, and a
        // tile is a thin slab, so that the walk does skip
        const int site[3] = {i % 10, i / 10 % 10, i / 100};
        for (int k = 0; k < 3; ++k) {
            const double x = (site[k] + 0.3 + 0.4 * u(rng)) * 0.1 * L;
            const double w = 2.0 * u(rng) - 1.0;
            s.pos[(size_t)k * s.P + i] = x;
            s.vel[(size_t)k * s.P + i] = w;
            s.xyz.push_back(x);
            s.v.push_back(w);
        }
    }
    return s;
}

ResidentView view_of(const System &s, bool compact = true)
{
    ResidentView v;
    v.n = s.n; v.P = s.P; v.TB = s.T; v.T = s.T; v.G = 1; v.rank = 0;
    v.L = s.L; v.invL = 1.0 / s.L; v.rc2 = s.rc * s.rc;
    v.pos = s.pos.data();
    v.v = s.vel.data();
    v.stream = nullptr;
    v.compact = compact;
    return v;
}

// E, P and C of the definition over the particles and the ordered pairs (i, j != i), in particle order
void brute(const System &s, uint64_t (&row)[9][3], bool &bad)
{
    std::memset(row, 0, sizeof row);
    for (int i = 0; i < s.n; ++i) {
        const double *w = &s.v[3 * (size_t)i];
        __int128 k[3] = {}, acc[6] = {};
        kinetic_terms(w[0], w[1], w[2], k, bad);
        for (int j = 0; j < s.n; ++j)
            if (j != i)
                pair_terms(&s.xyz[3 * (size_t)i], &s.xyz[3 * (size_t)j], w, &s.v[3 * (size_t)j], s.L, 1.0 / s.L, s.rc * s.rc, acc, bad);
        for (int c = 0; c < 3; ++c) add128(row[c], k[c]);
        for (int c = 0; c < 6; ++c) add128(row[3 + c], acc[c]);
    }
}

void guards_and_sequences()
{
    const System s = make_system(300, 8, 10.0, 2.5, 1);
    const ResidentView v = view_of(s);
    HeatfluxState st;
    std::string err;
    std::vector<int64_t> words(4 * kHeatfluxWords, -1);
    std::vector<double> j(4 * 3, -1.0), parts(4 * 9, -1.0);
    int64_t snaps = -1, vis = -1, tot = -1;
    double ms = -1.0;
    const char *who = "caller";

    // before configure
    check(heatflux_accumulate(&st, &err, who, v) == LJMD_ERR_STATE && has(err, "caller: the heat flux is not configured"),
          "accumulate before configure");
    check(heatflux_fetch(&st, &err, who, v, words.data(), &snaps) == LJMD_ERR_STATE && has(err, "not configured"), "read_exact before configure");
    check(heatflux_read(&st, &err, who, v, j.data(), parts.data(), &snaps) == LJMD_ERR_STATE && has(err, "not configured"), "read before configure");
    check(heatflux_reset(&st, &err, who, v) == LJMD_ERR_STATE && has(err, "not configured"), "reset before configure");
    check(heatflux_profile_read(&st, &err, who, v, &vis, &tot, &ms) == LJMD_ERR_STATE, "profile_read before configure");
    check(g_boxes + g_pairs + g_kinetic + g_fold == 0, "nothing launched before configure");
    heatflux_release(&st, nullptr);                          // what ljmd_destroy does on a handle never configured

    // guards of configure in their order, each leaving what was there
    ResidentView two = v, multi = v, big = v;
    two.G = 2; two.rank = 1; two.T = 2 * v.TB;
    multi.multi = true; multi.G = 2;
    big.n = kHeatfluxMaxN + 1;
    check(heatflux_configure(&st, &err, who, two, -1) == LJMD_ERR_INVALID_ARG && has(err, "caller: max_snapshots = -1 outside 1..262144"),
          "max_snapshots < 0 comes before the rank guard");
    check(heatflux_configure(&st, &err, who, v, kHeatfluxMaxSnapshots + 1) == LJMD_ERR_INVALID_ARG && has(err, "max_snapshots = 262145"),
          "max_snapshots too large");
    two.n = kHeatfluxMaxN + 1;
    check(heatflux_configure(&st, &err, who, two, 4) == LJMD_ERR_INVALID_ARG && has(err, "caller: n_ranks = 2: a pair term needs the velocities of both particles") &&
              has(err, "one-rank engine (ljmd_create with n_ranks = 1)"), "a rank engine is refused, before n is looked at");
    check(heatflux_configure(&st, &err, who, multi, 4) == LJMD_ERR_INVALID_ARG && has(err, "caller: n_ranks = 2 (multi-device handle): a pair term"),
          "a multi-device view is refused");
    check(heatflux_configure(&st, &err, who, big, 4) == LJMD_ERR_INVALID_ARG && has(err, "caller: n = 8388609 outside 1..8388608"), "n too large");
    check(st.max_snapshots == 0 && !st.d_series && !st.d_part && !st.d_bbox, "refused configure allocates nothing");
    check(heatflux_configure(&st, &err, who, big, 0) == LJMD_OK && heatflux_configure(&st, &err, who, two, 0) == LJMD_OK &&
              heatflux_configure(&st, &err, who, multi, 0) == LJMD_OK, "off needs no valid n and no one-rank engine");

    check(heatflux_configure(&st, &err, who, v, 3) == LJMD_OK && st.max_snapshots == 3 && st.d_series && st.d_part && st.d_kpart &&
              st.d_bbox && st.d_range && st.workgroups >= 1 && st.blocks == 1, "configure");
    check(heatflux_configure(&st, &err, who, v, -5) == LJMD_ERR_INVALID_ARG && st.max_snapshots == 3, "a refused reconfigure keeps the configuration");
    check(heatflux_configure(&st, &err, who, multi, 2) == LJMD_ERR_INVALID_ARG && st.max_snapshots == 3, "... for the rank guard too");
    check(heatflux_fetch(&st, &err, who, v, words.data(), &snaps) == LJMD_OK && snaps == 0 && words[0] == -1, "an empty series copies nothing");
    check(heatflux_profile_read(&st, &err, who, v, &vis, &tot, &ms) == LJMD_OK && vis == 0 && tot == 0 && ms == 0.0,
          "profile before the first accumulate");

    // the words against brute force
    uint64_t want[9][3];
    bool bad = false;
    brute(s, want, bad);
    check(!bad, "the test system is in range");
    check(heatflux_accumulate(&st, &err, who, v) == LJMD_OK && g_boxes == 1 && g_pairs == 1 && g_kinetic == 1 && g_fold == 1,
          "accumulate: four launches");
    check(g_last.skip == 1 && g_last.pos == v.pos && g_last.vel == v.v && g_last.bbox == st.d_bbox && g_last.L == 10.0 &&
              g_last.rc2 == 6.25 && g_last.T == 8 && g_last.P == 512, "accumulate: arguments");
    check(heatflux_fetch(&st, &err, who, v, words.data(), &snaps) == LJMD_OK && snaps == 1 &&
              std::memcmp(words.data(), want, sizeof want) == 0, "one snapshot equals the brute-force sum");
    check(words[kHeatfluxWords] == -1, "read_exact writes the taken snapshots only");
    check(heatflux_profile_read(&st, &err, who, v, &vis, &tot, &ms) == LJMD_OK && tot == 8 * 4 + 4 && vis > 0 && vis < tot,
          "profile: T (T / 2) + T / 2 tile pairs considered, some skipped");
    check(heatflux_profile_read(&st, &err, who, v, nullptr, nullptr, nullptr) == LJMD_OK, "profile with NULL pointers");
    check(heatflux_fetch(&st, &err, who, v, nullptr, nullptr) == LJMD_OK && heatflux_read(&st, &err, who, v, nullptr, nullptr, nullptr) == LJMD_OK,
          "reads with NULL pointers");

    // doubles: ljmd_heatflux_from_exact on the same words
    double j1[3], p1[9], j2[3] = {-1.0, -1.0, -1.0};
    check(heatflux_read(&st, &err, who, v, j.data(), parts.data(), &snaps) == LJMD_OK && snaps == 1 && j[3] == -1.0 && parts[9] == -1.0, "read");
    check(ljmd_heatflux_from_exact(words.data(), 10.0, j1, p1) == LJMD_OK && std::memcmp(j1, j.data(), sizeof j1) == 0 &&
              std::memcmp(p1, parts.data(), sizeof p1) == 0, "read = ljmd_heatflux_from_exact of read_exact");
    check(heatflux_read(&st, &err, who, v, j2, nullptr, nullptr) == LJMD_OK && std::memcmp(j1, j2, sizeof j1) == 0, "read without parts");
    std::vector<double> p2(9, -1.0);
    check(heatflux_read(&st, &err, who, v, nullptr, p2.data(), nullptr) == LJMD_OK && std::memcmp(p1, p2.data(), sizeof p1) == 0, "read without j");
    check(ljmd_heatflux_from_exact(words.data(), 10.0, j2, nullptr) == LJMD_OK && std::memcmp(j1, j2, sizeof j1) == 0, "from_exact without parts");
    for (int a = 0; a < 3; ++a)
        check(std::isfinite(j1[a]) && p1[a] != 0.0 && p1[3 + a] != 0.0 && p1[6 + a] != 0.0, "j is finite, no part is empty");
    check(ljmd_heatflux_from_exact(nullptr, 10.0, j1, p1) == LJMD_ERR_INVALID_ARG && ljmd_heatflux_from_exact(words.data(), 10.0, nullptr, p1) == LJMD_ERR_INVALID_ARG &&
              ljmd_heatflux_from_exact(words.data(), 0.0, j1, p1) == LJMD_ERR_INVALID_ARG && ljmd_heatflux_from_exact(words.data(), NAN, j1, p1) == LJMD_ERR_INVALID_ARG,
          "ljmd_heatflux_from_exact: guards");

    // not compact: nothing may be skipped, the same words
    check(heatflux_accumulate(&st, &err, who, view_of(s, false)) == LJMD_OK && g_last.skip == 0, "positions not compact: skip off");
    check(heatflux_profile_read(&st, &err, who, v, &vis, &tot, &ms) == LJMD_OK && vis == tot, "not compact: visited = total");
    check(heatflux_fetch(&st, &err, who, v, words.data(), &snaps) == LJMD_OK && snaps == 2 &&
              std::memcmp(words.data() + kHeatfluxWords, want, sizeof want) == 0, "the second row equals the first");

    // a failed launch: reported, not counted
    g_fail_pairs = 1;
    check(heatflux_accumulate(&st, &err, who, v) == LJMD_ERR_HIP && has(err, "caller: heat flux launch failed"), "failed launch");
    check(heatflux_fetch(&st, &err, who, v, nullptr, &snaps) == LJMD_OK && snaps == 2, "failed launch adds no snapshot");

    // a full series
    check(heatflux_accumulate(&st, &err, who, v) == LJMD_OK, "third snapshot");
    const int launches = g_boxes + g_pairs + g_kinetic + g_fold;
    check(heatflux_accumulate(&st, &err, who, v) == LJMD_ERR_STATE && has(err, "caller: the series is full (3 snapshots") &&
              has(err, "ljmd_heatflux_reset"), "full series");
    check(g_boxes + g_pairs + g_kinetic + g_fold == launches, "a full series launches nothing");
    check(heatflux_fetch(&st, &err, who, v, words.data(), &snaps) == LJMD_OK && snaps == 3, "full series reads");
    check(heatflux_reset(&st, &err, who, v) == LJMD_OK && heatflux_fetch(&st, &err, who, v, nullptr, &snaps) == LJMD_OK && snaps == 0, "reset empties");
    check(heatflux_accumulate(&st, &err, who, v) == LJMD_OK, "room again after reset");

    // an engine of another shape, or of more ranks
    const System other = make_system(600, 12, 10.0, 2.5, 2);
    check(heatflux_accumulate(&st, &err, who, view_of(other)) == LJMD_ERR_STATE && has(err, "not the one the heat flux was configured for"),
          "a view of another shape is refused");
    ResidentView ranked = v;
    ranked.G = 2; ranked.T = 2 * v.TB;
    const int before = g_pairs;
    check(heatflux_accumulate(&st, &err, who, ranked) == LJMD_ERR_STATE && g_pairs == before, "a rank view never reaches the kernels");

    // reconfigure empties, off frees
    check(heatflux_configure(&st, &err, who, v, 2) == LJMD_OK && st.max_snapshots == 2 && st.snapshots == 0, "reconfigure");
    check(heatflux_configure(&st, &err, who, v, 0) == LJMD_OK && st.max_snapshots == 0 && !st.d_series && !st.d_part && !st.d_kpart &&
              !st.d_bbox && !st.timer.ev0 && !st.timer.ev1, "off frees");
    check(heatflux_accumulate(&st, &err, who, v) == LJMD_ERR_STATE && heatflux_fetch(&st, &err, who, v, nullptr, nullptr) == LJMD_ERR_STATE,
          "off: as before configure");
    check(heatflux_configure(&st, &err, who, v, 2) == LJMD_OK && heatflux_accumulate(&st, &err, who, v) == LJMD_OK, "configured again");
    heatflux_release(&st, nullptr);                          // what ljmd_destroy does on a configured handle
    check(st.max_snapshots == 0 && !st.d_series, "release");
    heatflux_release(&st, nullptr);
}

// odd and even tile counts, one slice and many (LJMD_WALK_CHUNK), wide boxes: always the brute-force integers
void walks_against_brute_force()
{
    struct Case { int n, T; double rc; int chunk; };
    const Case cases[] = {{200, 5, 2.5, 0}, {256, 4, 4.9, 0}, {130, 3, 1.2, 0}, {64, 1, 4.9, 0}, {2, 1, 4.9, 0},
                          {500, 8, 2.5, 1}, {500, 8, 2.5, 3}, {450, 9, 4.9, 2}};
    for (const Case &c : cases) {
        const System s = make_system(c.n, c.T, 10.0, c.rc, 100 + c.n);
        ResidentView v = view_of(s);
        if (c.chunk) v.walk_chunk = c.chunk;
        HeatfluxState st;
        std::string err;
        uint64_t want[9][3];
        int64_t got[kHeatfluxWords];
        bool bad = false;
        brute(s, want, bad);
        check(heatflux_configure(&st, &err, "w", v, 1) == LJMD_OK && heatflux_accumulate(&st, &err, "w", v) == LJMD_OK &&
                  heatflux_fetch(&st, &err, "w", v, got, nullptr) == LJMD_OK && std::memcmp(got, want, sizeof want) == 0,
              "the walk equals the brute-force sum");
        check((int)(g_grid.x * g_grid.y) == st.workgroups && (!c.chunk || g_last.chunk == c.chunk), "the grid is the plan configure sized for");
        check(!bad, "walk cases are in range");
        heatflux_release(&st, nullptr);
    }
}

// a pair 1e-4 apart: its terms enter as 0, the sticky word is set until reset, nothing else is disturbed; then a velocity
void range_flag()
{
    System s = make_system(128, 2, 10.0, 2.5, 9);
    for (int k = 0; k < 3; ++k) s.pos[(size_t)k * s.P + 1] = s.pos[(size_t)k * s.P] + (k == 0 ? 1e-4 : 0.0);
    for (int k = 0; k < 3; ++k) s.xyz[3 + k] = s.pos[(size_t)k * s.P + 1];
    const ResidentView v = view_of(s);
    HeatfluxState st;
    std::string err;
    uint64_t want[9][3];
    int64_t got[kHeatfluxWords];
    int64_t snaps = -1;
    bool bad = false;
    brute(s, want, bad);
    check(bad, "1e-4 apart is out of range");
    check(heatflux_configure(&st, &err, "g", v, 4) == LJMD_OK && heatflux_accumulate(&st, &err, "g", v) == LJMD_OK, "accumulate succeeds");
    check(heatflux_fetch(&st, &err, "g", v, got, &snaps) == LJMD_ERR_RANGE && has(err, "g: a pair's or a particle's heat flux terms") &&
              has(err, "until ljmd_heatflux_reset") && snaps == -1, "read_exact: LJMD_ERR_RANGE");
    check(std::memcmp(got, want, sizeof want) == 0, "the flagged pair entered as zeros, everything else as usual");
    double j[3];
    check(heatflux_read(&st, &err, "g", v, j, nullptr, nullptr) == LJMD_ERR_RANGE, "read: LJMD_ERR_RANGE");
    check(heatflux_accumulate(&st, &err, "g", v) == LJMD_OK && heatflux_fetch(&st, &err, "g", v, nullptr, nullptr) == LJMD_ERR_RANGE, "sticky");
    check(heatflux_reset(&st, &err, "g", v) == LJMD_OK && heatflux_fetch(&st, &err, "g", v, nullptr, &snaps) == LJMD_OK && snaps == 0,
          "reset clears the word");
    // k2 v out of range: 2^15 squared is 2^30, times 2^15 is 2^45
    s.vel[5] = 0x1p15;
    s.v[3 * 5] = 0x1p15;
    s.pos[1] = NAN;                                          // the close pair is gone: slot 1 fails every cutoff test now
    s.xyz[3] = NAN;
    bad = false;
    brute(s, want, bad);
    check(bad, "a velocity of 2^15 is out of range");
    check(heatflux_accumulate(&st, &err, "g", v) == LJMD_OK && heatflux_fetch(&st, &err, "g", v, got, nullptr) == LJMD_ERR_RANGE &&
              std::memcmp(got, want, sizeof want) == 0, "a convective term of 2^45 sets the word and enters as 0");
    heatflux_release(&st, nullptr);
}

}  // namespace

int main()
{
    setenv("FAKEHIP_DEVICES", "1", 1);
    guards_and_sequences();
    walks_against_brute_force();
    range_flag();
    if (g_failures == 0) std::printf("heatflux_host: ok\n");
    return g_failures == 0 ? 0 : 1;
}
