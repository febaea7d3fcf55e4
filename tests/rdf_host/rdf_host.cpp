// rdf_host.cpp -- TEST INFRASTRUCTURE: the host core of the engine's resident g(r) (csrc/ljmd_rdf.cpp, namespace ljmdr)
// without a GPU and without the engine.  Linked from the core, ljmd_common.cpp, the fake HIP runtime (tests/fakehip) and
// its own definitions of the two launchers, which check what they are given and add known numbers where the kernels
// would add counts.  The program checks itself -- every guard with its return code and message, the sequences around
// configure / accumulate / read / reset, the bound that keeps a 32-bit LDS bin from overflowing for n up to 2^23, and
// the tile-pair bound of ljmd_rdf.h against brute force, and the walk itself: the loop structure of rdf_pairs_kernel /
// stress_pairs_kernel (slices, blocks of 64 steps, lanes, rdf_walk_column and rdf_walk_takes) replayed for a grid of
// shapes and LJMD_WALK_CHUNK values, every tile pair counted -- prints one line per check that fails and "rdf_host: ok" when
// none did.  tests/test_rdf_host.py runs it under ASan and UBSan.  (The fake hipMalloc cannot fail, so the
// LJMD_ERR_ALLOC branch of configure is not reached here.)
#include "ljmd.h"
#include "ljmd_common.h"
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

using namespace ljmdr;

namespace {

int g_failures = 0;
int g_boxes = 0, g_pairs = 0;
int g_fail_pairs = 0;                      // 1: the next pair launch returns hipErrorLaunchFailure
RdfPairArgs g_last{};
dim3 g_grid;

void check(bool ok, const char *what)
{
    if (ok) return;
    ++g_failures;
    std::printf("FAILED: %s\n", what);
}

bool has(const std::string &err, const char *text) { return err.find(text) != std::string::npos; }

}  // namespace

namespace ljmdr {

hipError_t launch_rdf_boxes(const RdfBoxArgs &a, hipStream_t)
{
    ++g_boxes;
    check(a.pos && a.bbox && a.T >= 1 && a.TB >= 1 && a.T % a.TB == 0, "box launch: arguments");
    for (int t = 0; t < a.T * kRdfBoxStride; ++t) a.bbox[t] = 1.0;      // the buffer holds T boxes
    return hipSuccess;
}

hipError_t launch_rdf_pairs(const RdfPairArgs &a, dim3 grid, hipStream_t)
{
    ++g_pairs;
    if (g_fail_pairs > 0 && --g_fail_pairs == 0) return hipErrorLaunchFailure;
    g_last = a;
    g_grid = grid;
    const int weight = a.G == 1 ? 2 : 1;
    check(a.nbins >= 1 && a.nbins <= kRdfMaxBins, "pair launch: nbins");
    check(a.T == a.G * a.TB && a.rank >= 0 && a.rank < a.G, "pair launch: tiles and rank");
    check(a.U == (a.G == 1 ? a.T / 2 + 1 : a.T), "pair launch: steps of the walk");
    check(a.chunk >= 1 && a.chunk <= kRdfMaxChunk && (long long)grid.y * a.chunk >= a.U &&
              (long long)(grid.y - 1) * a.chunk < a.U, "pair launch: the slices cover the walk, none is empty");
    check((long long)grid.x * kRdfWaves >= a.TB && (long long)(grid.x - 1) * kRdfWaves < a.TB, "pair launch: row blocks");
    check(rdf_lds_bound(a.chunk, weight) <= 0xffffffffull, "pair launch: a 32-bit bin cannot overflow");
    check(a.rmax2_skin > a.rmax * a.rmax && a.rmax2_up > a.rmax * a.rmax && a.rmax2_up < a.rmax2_skin,
          "pair launch: rmax^2 < prefilter bound < skip bound");
    check(a.dr == a.rmax / a.nbins && a.inv_dr == 1.0 / a.dr, "pair launch: dr = rmax / nbins, inv_dr = 1 / dr");
    a.hist[0] += 7;
    a.hist[a.nbins - 1] += 1;
    a.count[0] += 3;
    a.count[1] += 5;
    return hipSuccess;
}

}  // namespace ljmdr

namespace {

ResidentView view_for(int n, int G, int rank, std::vector<double> &pos)
{
    ResidentView v;
    v.n = n; v.G = G; v.rank = rank;
    v.S = n / G;
    v.P = (v.S + 255) / 256 * 256;
    v.TB = v.P / 64;
    v.T = G * v.TB;
    v.L = 10.0; v.invL = 0.1;
    pos.assign((size_t)G * 3 * v.P, 0.5);
    v.pos = pos.data();
    v.stream = nullptr;
    v.compact = true;
    return v;
}

void guards_and_sequences()
{
    std::vector<double> pos;
    const ResidentView v = view_for(1000, 1, 0, pos);
    RdfState st;
    std::string err;
    uint64_t hist[64];
    int64_t snaps = -1, vis = -1, tot = -1;
    double ms = -1.0;
    const char *who = "caller";

    // before configure
    check(rdf_accumulate(&st, &err, who, v) == LJMD_ERR_STATE && has(err, "caller: g(r) is not configured"), "accumulate before configure");
    check(rdf_read(&st, &err, who, v, hist, &snaps) == LJMD_ERR_STATE && has(err, "not configured"), "read before configure");
    check(rdf_reset(&st, &err, who, v) == LJMD_ERR_STATE && has(err, "not configured"), "reset before configure");
    check(rdf_profile_read(&st, &err, who, v, &vis, &tot, &ms) == LJMD_ERR_STATE, "profile_read before configure");
    check(g_boxes == 0 && g_pairs == 0, "nothing launched before configure");

    // guards of configure, each leaving what was there
    check(rdf_configure(&st, &err, who, v, -1, 1.0) == LJMD_ERR_INVALID_ARG && has(err, "caller: nbins = -1 outside 1..8192"), "nbins < 0");
    check(rdf_configure(&st, &err, who, v, kRdfMaxBins + 1, 1.0) == LJMD_ERR_INVALID_ARG && has(err, "nbins = 8193"), "nbins too large");
    const double bad[] = {0.0, -1.0, NAN, INFINITY, -INFINITY};
    for (double r : bad)
        check(rdf_configure(&st, &err, who, v, 10, r) == LJMD_ERR_INVALID_ARG && has(err, "caller: rmax must be finite and > 0"), "bad rmax");
    check(st.nbins == 0 && !st.d_hist && !st.d_bbox && !st.d_count, "refused configure allocates nothing");
    check(rdf_configure(&st, &err, who, v, 0, NAN) == LJMD_OK, "nbins = 0 ignores rmax");

    check(rdf_configure(&st, &err, who, v, 64, 7.0) == LJMD_OK && st.nbins == 64 && st.d_hist && st.d_bbox && st.d_count,
          "configure");                                      // rmax above L / 2 is allowed
    check(rdf_configure(&st, &err, who, v, 9000, 1.0) == LJMD_ERR_INVALID_ARG && st.nbins == 64 && st.rmax == 7.0,
          "a refused reconfigure keeps the configuration");
    check(rdf_configure(&st, &err, who, v, 32, NAN) == LJMD_ERR_INVALID_ARG && st.nbins == 64, "a refused rmax keeps it too");
    check(rdf_read(&st, &err, who, v, hist, &snaps) == LJMD_OK && snaps == 0 && hist[0] == 0 && hist[63] == 0, "zeroed by configure");
    check(rdf_profile_read(&st, &err, who, v, &vis, &tot, &ms) == LJMD_OK && vis == 0 && tot == 0 && ms == 0.0,
          "profile before the first accumulate");

    // snapshot counting; the stub adds 7 to bin 0 and 1 to the last bin per launch
    check(rdf_accumulate(&st, &err, who, v) == LJMD_OK && g_boxes == 1 && g_pairs == 1, "accumulate: two launches");
    check(g_last.skip == 1 && g_last.G == 1 && g_last.nbins == 64 && g_last.pos == v.pos && g_last.bbox == st.d_bbox &&
              g_last.hist == st.d_hist && g_last.L == 10.0 && g_last.rmax == 7.0, "accumulate: arguments");
    check(rdf_accumulate(&st, &err, who, v) == LJMD_OK, "accumulate again");
    check(rdf_read(&st, &err, who, v, hist, &snaps) == LJMD_OK && snaps == 2 && hist[0] == 14 && hist[63] == 2, "two snapshots");
    check(rdf_read(&st, &err, who, v, nullptr, nullptr) == LJMD_OK, "read with NULL pointers");
    check(rdf_read(&st, &err, who, v, hist, &snaps) == LJMD_OK && snaps == 2 && hist[0] == 14, "read clears nothing");
    check(rdf_profile_read(&st, &err, who, v, &vis, &tot, &ms) == LJMD_OK && vis == 3 && tot == 5,
          "profile: the counters of the most recent accumulate only");
    check(rdf_profile_read(&st, &err, who, v, nullptr, nullptr, nullptr) == LJMD_OK, "profile with NULL pointers");

    // a failed launch: reported, not counted
    g_fail_pairs = 1;
    check(rdf_accumulate(&st, &err, who, v) == LJMD_ERR_HIP && has(err, "caller: g(r) launch failed"), "failed launch");
    check(rdf_read(&st, &err, who, v, hist, &snaps) == LJMD_OK && snaps == 2 && hist[0] == 14, "failed launch adds no snapshot");

    check(rdf_reset(&st, &err, who, v) == LJMD_OK, "reset");
    check(rdf_read(&st, &err, who, v, hist, &snaps) == LJMD_OK && snaps == 0 && hist[0] == 0 && hist[63] == 0, "reset zeroes");

    // not compact: nothing may be skipped
    ResidentView loose = v;
    loose.compact = false;
    check(rdf_accumulate(&st, &err, who, loose) == LJMD_OK && g_last.skip == 0, "positions not compact: skip off");

    // reconfigure zeroes, off frees
    check(rdf_configure(&st, &err, who, v, 16, 2.0) == LJMD_OK && st.nbins == 16 && st.snapshots == 0, "reconfigure");
    check(rdf_read(&st, &err, who, v, hist, &snaps) == LJMD_OK && snaps == 0 && hist[0] == 0 && hist[15] == 0, "reconfigure zeroes");
    check(rdf_configure(&st, &err, who, v, 0, 0.0) == LJMD_OK && st.nbins == 0 && !st.d_hist && !st.d_bbox && !st.d_count &&
              !st.timer.ev0 && !st.timer.ev1, "off frees");
    check(rdf_accumulate(&st, &err, who, v) == LJMD_ERR_STATE && rdf_read(&st, &err, who, v, hist, &snaps) == LJMD_ERR_STATE,
          "off: as before configure");

    // a rank engine: ordered walk over all column tiles
    std::vector<double> pos4;
    const ResidentView rv = view_for(4096, 4, 2, pos4);
    check(rdf_configure(&st, &err, who, rv, 8192, 3.0) == LJMD_OK, "configure on a rank view");
    check(rdf_accumulate(&st, &err, who, rv) == LJMD_OK && g_last.G == 4 && g_last.rank == 2 && g_last.U == rv.T &&
              g_last.TB == rv.TB, "rank view: arguments");
    rdf_release(&st, nullptr);                               // what ljmd_destroy does on a configured handle
    check(st.nbins == 0 && !st.d_hist, "release");
    rdf_release(&st, nullptr);                               // and on one that is not
}

// the LDS bins: whatever the system, a slice adds less than 2^32 to a bin and the slices cover the walk
void overflow_bound()
{
    const int ns[] = {2, 64, 65, 1000, 4096, 262144, 1048576, (1 << 23) - 64, 1 << 23};
    const int Gs[] = {1, 2, 4, 8, 64};
    for (int n : ns)
        for (int G : Gs) {
            if (n % G) continue;
            const int S = n / G, P = (S + 255) / 256 * 256, TB = P / 64, T = G * TB;
            const RdfWalk w = rdf_plan_walk(TB, T, G, std::nullopt);
            const bool ok = w.weight == (G == 1 ? 2 : 1) && w.U == (G == 1 ? T / 2 + 1 : T) && w.chunk >= 1 &&
                            w.chunk <= kRdfMaxChunk && (long long)w.slices * w.chunk >= w.U &&
                            (long long)(w.slices - 1) * w.chunk < w.U && w.row_blocks * kRdfWaves >= TB &&
                            rdf_lds_bound(w.chunk, w.weight) <= 0xffffffffull;
            if (!ok) std::printf("walk of n = %d, G = %d: U %d chunk %d slices %d\n", n, G, w.U, w.chunk, w.slices);
            check(ok, "walk plan");
        }
    check(rdf_lds_bound(kRdfMaxChunk, 2) == (1ull << 31), "the largest slice adds 2^31 at most");
    check(rdf_lds_bound(2 * kRdfMaxChunk, 2) > 0xffffffffull, "twice the largest slice would not fit");
}

// ---- the walk, enumerated ----
// What the replay saw, so that none of the paths it is there for is vacuous.
struct WalkSeen {
    bool second_block = false;      // a slice longer than 64 steps
    bool partial_block = false;     // a last block with fewer than 64 steps, after a full one
    bool full_last_block = false;   // u1 == ub + 64 exactly
    bool tie_later_block = false;   // the tie step of an even T in a block other than a slice's first, taken and dropped
    bool tie_dropped_later = false;
    bool wrap_later_block = false;  // J wrapped at T in a block other than the first
    bool own_tile_later = false;    // the own tile of the ordered walk in a block other than the first
    bool odd_T = false;
} g_seen;

// One launch of the pair kernels for `rank`, as they walk: grid (row_blocks, slices), kRdfWaves waves per workgroup, each
// taking its slice 64 steps at a time, one lane per step; every lane's box test kept (skip off), then the set bits
// walked.  count[I T + J] += 1 per evaluated tile pair; -> the `considered` popcounts.
long long replay_walk(int TB, int T, int G, int rank, const RdfWalk &w, std::vector<unsigned char> &count)
{
    const bool unordered = G == 1;
    long long considered = 0;
    for (int by = 0; by < w.slices; ++by)
        for (int bx = 0; bx < w.row_blocks; ++bx)
            for (int wave = 0; wave < kRdfWaves; ++wave) {
                const int Il = bx * kRdfWaves + wave;
                if (Il >= TB) continue;
                const int I = rank * TB + Il;
                const int u0 = by * w.chunk, u1 = std::min(u0 + w.chunk, w.U);
                check(u0 < u1, "walk: no slice is empty");
                for (int ub = u0; ub < u1; ub += 64) {
                    uint64_t m = 0;
                    int Jlane[64];
                    for (int lane = 0; lane < 64; ++lane) {
                        const int u = ub + lane;
                        Jlane[lane] = rdf_walk_column(I, u, T, unordered);
                        if (!rdf_walk_takes(I, u, u1, T, unordered)) {
                            if (u < u1 && ub > u0) g_seen.tie_dropped_later = true;
                            continue;
                        }
                        check(Jlane[lane] >= 0 && Jlane[lane] < T && u < w.U, "walk: a valid lane names a tile of the system");
                        m |= 1ull << lane;
                    }
                    considered += __builtin_popcountll(m);
                    if (ub > u0) g_seen.second_block = true;
                    if (ub > u0 && u1 - ub < 64) g_seen.partial_block = true;
                    if (u1 - ub == 64) g_seen.full_last_block = true;
                    while (m) {
                        const int b = __builtin_ctzll(m);
                        m &= m - 1;
                        const int Jb = rdf_walk_column(I, ub + b, T, unordered);
                        check(Jb == Jlane[b], "walk: the evaluated tile is the tested one");
                        if (Jb < 0 || Jb >= T) continue;
                        unsigned char &c = count[(size_t)I * T + Jb];
                        if (c < 255) ++c;
                        if (ub > u0) {
                            if (unordered && (T & 1) == 0 && ub + b == T / 2) g_seen.tie_later_block = true;
                            if (unordered && I + ub + b >= T) g_seen.wrap_later_block = true;
                            if (!unordered && Jb == I) g_seen.own_tile_later = true;
                        }
                    }
                }
            }
    return considered;
}

void walk_enumeration()
{
    const int TBs[] = {1, 4, 5, 33, 36, 64, 65, 132, 260};
    const int Gs[] = {1, 2, 3, 4, 8};
    for (int TB : TBs)
        for (int G : Gs) {
            const int T = G * TB, U = G == 1 ? T / 2 + 1 : T;
            if (T & 1) g_seen.odd_T = true;
            const int chunks[] = {1, 2, 63, 64, 65, U - 1, U, U + 7};
            for (int chunk : chunks) {
                const RdfWalk w = rdf_plan_walk(TB, T, G, chunk);
                const bool plan_ok = w.U == U && w.chunk == std::max(1, std::min(chunk, std::min(U, kRdfMaxChunk))) &&
                                     w.slices == (U + w.chunk - 1) / w.chunk && w.row_blocks == (TB + kRdfWaves - 1) / kRdfWaves &&
                                     w.weight == (G == 1 ? 2 : 1);
                if (!plan_ok) std::printf("TB %d G %d asked %d: U %d chunk %d slices %d\n", TB, G, chunk, w.U, w.chunk, w.slices);
                check(plan_ok, "walk: the plan under an override");
                // rows I of the array are written by the rank that owns them and by no other
                std::vector<unsigned char> all((size_t)T * T, 0);
                bool ok = true;
                long long considered = 0;
                for (int rank = 0; rank < G; ++rank) {
                    const long long con = replay_walk(TB, T, G, rank, w, all);
                    considered += con;
                    if (G > 1) ok = ok && con == (long long)TB * T;      // own rows x every column
                }
                if (G == 1) {
                    // every unordered tile pair from one side only, every diagonal tile once
                    for (int I = 0; I < T; ++I) {
                        ok = ok && all[(size_t)I * T + I] == 1;
                        for (int J = I + 1; J < T; ++J) ok = ok && all[(size_t)I * T + J] + all[(size_t)J * T + I] == 1;
                    }
                    ok = ok && considered == ((T & 1) ? (long long)T * (T / 2 + 1) : (long long)T * (T / 2) + T / 2);
                } else {
                    // every rank every ordered tile pair of its rows once; together all T x T
                    ok = ok && std::count(all.begin(), all.end(), (unsigned char)1) == (long long)T * T;
                    ok = ok && considered == (long long)T * T;
                }
                if (!ok) std::printf("TB %d G %d chunk %d (asked %d): considered %lld\n", TB, G, w.chunk, chunk, considered);
                check(ok, "walk: every tile pair exactly once, `considered` the closed form");
            }
        }
    check(g_seen.second_block && g_seen.partial_block && g_seen.full_last_block && g_seen.tie_later_block &&
              g_seen.tie_dropped_later && g_seen.wrap_later_block && g_seen.own_tile_later && g_seen.odd_T,
          "walk: the grid reached every path it is there for");
    // unset and out-of-range requests
    const RdfWalk plain = rdf_plan_walk(132, 132, 1, std::nullopt);
    check(plain.chunk == 1 && plain.slices == 67, "walk: unset, T = 132 is one step per slice");
    check(rdf_plan_walk(132, 132, 1, 0).chunk == 1 && rdf_plan_walk(132, 132, 1, -5).chunk == 1 &&
              rdf_plan_walk(132, 132, 1, 1000).chunk == 67 && rdf_plan_walk(132, 132, 1, 1000).slices == 1,
          "walk: a request is clamped to [1, U]");
    // from the environment to the launch: read_knobs -> (the handle's Knobs) -> ResidentView -> the grid of rdf_accumulate
    setenv("LJMD_WALK_CHUNK", "65", 1);
    const std::optional<int> knob = ljmdh::read_knobs().walk_chunk;
    unsetenv("LJMD_WALK_CHUNK");
    check(knob && *knob == 65 && !ljmdh::read_knobs().walk_chunk, "walk: read_knobs reads LJMD_WALK_CHUNK, unset is unset");
    std::vector<double> pos;
    ResidentView v = view_for(8200, 1, 0, pos);
    v.walk_chunk = knob;
    RdfState st;
    std::string err;
    check(rdf_configure(&st, &err, "k", v, 16, 2.0) == LJMD_OK && rdf_accumulate(&st, &err, "k", v) == LJMD_OK &&
              g_last.chunk == 65 && g_last.U == 67 && g_grid.y == 2 && g_grid.x == 33, "walk: accumulate launches the overridden plan");
    v.walk_chunk = std::nullopt;
    check(rdf_accumulate(&st, &err, "k", v) == LJMD_OK && g_last.chunk == 1 && g_grid.y == 67, "walk: unset, the plan of before");
    rdf_release(&st, nullptr);
    const int bigT = 4 * kRdfMaxChunk;
    check(rdf_plan_walk(bigT, bigT, 1, 1 << 30).chunk == kRdfMaxChunk, "walk: a request is clamped to kRdfMaxChunk");
    check(rdf_lds_bound(rdf_plan_walk(bigT, bigT, 1, 1 << 30).chunk, 2) <= 0xffffffffull, "walk: a clamped request keeps the LDS bound");
}

// ---- the tile-pair bound against brute force ----
struct Box {
    double b[6];
};

// the pair pass's distance (rdf_image's integer is rint(d / L); its fast path returns the same integer)
double pair_r(const double *pi, const double *pj, double L)
{
    double d[3];
    for (int k = 0; k < 3; ++k) {
        d[k] = pj[k] - pi[k];
        d[k] = d[k] - L * std::nearbyint(d[k] / L);
    }
    return std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
}

long g_skipped = 0, g_kept = 0;

void probe(const Box &bi, const Box &bj, double L, double rmax, std::mt19937_64 &rng)
{
    const double skin = rmax * rmax * (1.0 + 1e-10);
    const bool skipped = rdf_tile_gap2(bi.b, bj.b, L) > skin;
    check(skipped == (rdf_tile_gap2(bj.b, bi.b, L) > skin), "the bound is symmetric");
    if (!skipped) {
        ++g_kept;
        return;
    }
    ++g_skipped;
    // sample points: the 8 corners, then points on faces and inside
    std::uniform_real_distribution<double> u(0.0, 1.0);
    std::vector<double> pi, pj;
    auto fill = [&](const Box &b, std::vector<double> &p) {
        for (int c = 0; c < 8; ++c)
            for (int k = 0; k < 3; ++k) p.push_back(b.b[(c >> k & 1) ? 3 + k : k]);
        for (int s = 0; s < 24; ++s) {
            const int pin = s % 4;              // 0..2: that axis pinned to a face; 3: interior
            for (int k = 0; k < 3; ++k) {
                const double t = (k == pin) ? (s & 4 ? 1.0 : 0.0) : u(rng);
                double x = b.b[k] + t * (b.b[3 + k] - b.b[k]);
                x = std::fmin(std::fmax(x, b.b[k]), b.b[3 + k]);
                p.push_back(x);
            }
        }
    };
    fill(bi, pi);
    fill(bj, pj);
    for (size_t a = 0; a < pi.size(); a += 3)
        for (size_t c = 0; c < pj.size(); c += 3)
            if (pair_r(&pi[a], &pj[c], L) < rmax) {
                std::printf("skipped tile pair holds r = %.17g < rmax = %.17g (L = %.17g)\n", pair_r(&pi[a], &pj[c], L), rmax, L);
                check(false, "a skipped tile pair contains no pair within rmax");
                return;
            }
}

void gap_bound_property()
{
    std::mt19937_64 rng(20240607);
    std::uniform_real_distribution<double> u(0.0, 1.0);
    const double Ls[] = {4.0, 17.235477520255067, 68.94};
    for (double L : Ls) {
        // compact positions: every coordinate inside one window narrower than 2.4 L
        const double w0 = -0.7 * L, w1 = 1.69 * L;
        auto random_box = [&](double max_side) {
            Box b;
            for (int k = 0; k < 3; ++k) {
                const double side = u(rng) * max_side;
                const double lo = w0 + u(rng) * (w1 - w0 - side);
                b.b[k] = lo;
                b.b[3 + k] = lo + side;
            }
            return b;
        };
        for (int trial = 0; trial < 4000; ++trial) {
            const double rmax = (0.01 + 0.89 * u(rng)) * L;
            const int kind = trial % 8;
            Box bi = random_box(kind == 0 ? 0.9 * L : 0.3 * L), bj = random_box(kind == 1 ? 0.9 * L : 0.3 * L);
            if (kind == 2)                          // single points
                for (int k = 0; k < 3; ++k) { bi.b[3 + k] = bi.b[k]; bj.b[3 + k] = bj.b[k]; }
            if (kind == 3) {                        // touching the faces of the box from both sides
                bi.b[0] = 0.0; bi.b[3] = 0.1 * L; bj.b[3] = L; bj.b[0] = 0.85 * L;
            }
            if (kind == 4) {                        // straddling a face
                bi.b[1] = -0.05 * L; bi.b[4] = 0.05 * L;
            }
            if (kind == 5) {                        // exactly half a box apart on one axis
                bj.b[2] = bi.b[2] + 0.5 * L; bj.b[5] = bj.b[2];
                bi.b[5] = bi.b[2];
            }
            if (kind == 6) {                        // the gap equal to rmax on one axis, zero on the others
                bj = bi;
                bj.b[0] = bi.b[3] + rmax; bj.b[3] = bj.b[0] + 0.1 * L;
                if (bj.b[3] > w1) continue;
            }
            if (kind == 7) {                        // an empty tile: never within reach of anything
                for (int k = 0; k < 3; ++k) { bj.b[k] = INFINITY; bj.b[3 + k] = -INFINITY; }
                check(rdf_tile_gap2(bi.b, bj.b, L) == INFINITY && rdf_tile_gap2(bj.b, bi.b, L) == INFINITY &&
                          rdf_tile_gap2(bj.b, bj.b, L) == INFINITY, "empty tiles are infinitely far");
                continue;
            }
            probe(bi, bj, L, rmax, rng);
        }
    }
    // the bound does skip, and does keep: neither side of the property is vacuous
    check(g_skipped > 1000 && g_kept > 1000, "the property test saw skipped and kept tile pairs");
    // beyond sqrt(3) L / 2 no pair of boxes is ever skipped
    Box a{{0, 0, 0, 0, 0, 0}}, b{{2.0, 2.0, 2.0, 2.0, 2.0, 2.0}};
    check(!(rdf_tile_gap2(a.b, b.b, 4.0) > 3.6 * 3.6), "rmax = 0.9 L reaches the farthest image");
    check(rdf_tile_gap2(a.b, b.b, 4.0) == 12.0, "opposite corners of the half box");
}

}  // namespace

int main()
{
    setenv("FAKEHIP_DEVICES", "1", 1);
    guards_and_sequences();
    overflow_bound();
    walk_enumeration();
    gap_bound_property();
    if (g_failures == 0) std::printf("rdf_host: ok\n");
    return g_failures == 0 ? 0 : 1;
}
