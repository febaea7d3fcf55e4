// ljmd_plan.cpp -- what an engine decides once, when it is created, from (n, n_ranks, precision mode) and the table of
// LJMD_* knobs (read_knobs, ljmd_common.cpp): the launch plan of its three kernel families.  Host arithmetic only: no HIP
// call and no getenv.
#include "ljmd_engine.h"

namespace ljmdh {

namespace {
// smallest m > 0 with m * uchunk a multiple of rt
int rt_align(int uchunk, int rt)
{
    int m = 1;
    while ((m * uchunk) % rt != 0) ++m;
    return m;
}
}  // namespace

int plan_engine(const SimParams &sim, int n, int n_ranks, int precision_mode, const Knobs &k, LaunchPlan *out)
{
    LaunchPlan p;
    p.S = n / n_ranks;
    p.P = ((p.S + kSlotAlign - 1) / kSlotAlign) * kSlotAlign;
    p.TB = p.P / kTile;
    p.T = n_ranks * p.TB;
    p.W = (p.T + 63) / 64;
    p.rc_allows_fast = sim.rc <= (1.0 - 1e-9) * 0.5 * sim.L;
    // below ~16 tiles there is nothing for the tile mask to skip: keep the caller's order
    p.sort_enabled = k.sort && n >= 1024;
    // tiles loosen as the particles diffuse while one re-sort costs ~1.2 ms at n = 262144: the larger the system, the
    // sooner a re-sort pays for itself (pair time per rank ~ n^2 / G, sort time ~ n / G: the ratio depends on n only).
    // (Most of the slow-down once measured between two sorts -- +9 % after 9 steps in the liquid -- came from tiles that
    // straddle a box face; the tile-coherent positions of tile_boxes_kernel removed it, and 10 / 15 / 20 / 30 steps now
    // differ by < 3 % at n = 262144.)
    // Small systems (n <= 8192): one re-sort is ~30 launches = 135 us against a 33 us step, and in 200 steps a particle of
    // the liquid moves ~0.5 sigma against tiles of 4.3 sigma: every 200 steps (20: 25 300 steps/s at n = 4096, 100: 29 500,
    // 200: 30 000, 400: 30 500 -- tools/small_n_rate.py, profiles/r03_small_n_two_launch_step.txt).
    // Round 4 (profiles/r04_resort_interval_mid_n.txt): the same holds up to the end of the two-launch regime -- n = 12 288:
    // 8225 steps/s at 20, 8929 at 200; 16 384: 5875 / 6130 -- where nearly every tile pair is inside the cutoff anyway; 50 up
    // to 40 000 (32 768: 2134 / 2158), 20 beyond (65 536: 657 at 20, 645 at 200).
    p.resort_every = std::max(1, k.resort_every.value_or(n >= 1000000 ? 5 : n >= 131072 ? 10 : n > 40000 ? 20
                                                              : n > kFuseTailMaxN ? 50 : 200));
    {   // k-d levels: segments = runs of whole tiles, halved until every segment is one tile
        const int tiles = (p.S + kTile - 1) / kTile;
        std::vector<int> bounds = {0, tiles};
        while (true) {
            bool any = false;
            for (size_t j = 0; j + 1 < bounds.size(); ++j) any = any || (bounds[j + 1] - bounds[j] > 1);
            if (!any) break;
            p.kd_level_off.push_back(p.kd_offsets.size());
            p.kd_level_nseg.push_back((int)bounds.size() - 1);
            for (int b : bounds) p.kd_offsets.push_back(std::min(b * kTile, p.S));
            std::vector<int> next;
            for (size_t j = 0; j + 1 < bounds.size(); ++j) {
                next.push_back(bounds[j]);
                const int t = bounds[j + 1] - bounds[j];
                if (t > 1) next.push_back(bounds[j] + (t + 1) / 2);
            }
            next.push_back(tiles);
            bounds.swap(next);
        }
        // the first level whose largest segment fits one workgroup of kd_finish_kernel: it and the later ones (segments
        // only shrink) are sorted there, the levels above by the library
        const int levels = (int)p.kd_level_nseg.size();
        p.kd_finish_from = levels;
        for (int l = levels - 1; l >= 0 && !k.kd_sort_cub; --l) {
            int largest = 0;
            for (int j = 0; j < p.kd_level_nseg[l]; ++j)
                largest = std::max(largest, p.kd_offsets[p.kd_level_off[l] + j + 1] - p.kd_offsets[p.kd_level_off[l] + j]);
            if (largest > kKdFinishCap) break;
            p.kd_finish_from = l;
        }
    }

    // launch geometry: rows x slices >= kTargetWorkgroups
    const int row_blocks = p.P / kBlock;
    {   // generic kernel: slices over the n real particles
        int ns = (kTargetWorkgroups + row_blocks - 1) / row_blocks;
        ns = std::max(1, std::min(ns, (n + 63) / 64));
        p.chunk_g = ((n + ns - 1) / ns + 7) / 8 * 8;
        p.nslab_g = (n + p.chunk_g - 1) / p.chunk_g;
    }
    {   // tile (gather) kernel: slices of column tiles
        int ns = (kTargetWorkgroups + row_blocks - 1) / row_blocks;
        ns = std::max(1, std::min(ns, p.T));
        p.chunk_t = (p.T + ns - 1) / ns;
        p.nslab_t = (p.T + p.chunk_t - 1) / p.chunk_t;
    }
    {   // Newton-3 kernel: NG row groups over all ranks, NGo owned; offsets 0..Dmax in slices
        // tiles per row group: 4 is the measured optimum when there is plenty of work; small systems take 2 or
        // 1 so that (row groups) x (offsets) still fills the 1024 SIMDs
        const bool mixed_mode = precision_mode == LJMD_PRECISION_FP32_FORCE;
        int rt = k.n3_row_tiles;
        if (mixed_mode) rt = kRowTiles;                       // the fp32 far kernel is built for 4
        if (rt != 1 && rt != 2 && rt != kRowTiles) {
            // measured (profiles/r04_unit_sweep.txt; work items cut down to single passes, N3Args::uchunk): 4 wins from
            // n = 32768 up, 2 from 6144 (two-launch step included), 1 below
            auto items = [&](int cand) { const long ngo = p.TB / cand; return ngo * ((long)n_ranks * ngo / 2 + 1); };
            rt = items(kRowTiles) >= kN3ItemsFor4 ? kRowTiles : items(2) >= kN3ItemsFor2 ? 2 : 1;
        }
        p.rt = rt;
        p.NGo = p.TB / rt;
        p.NG = n_ranks * p.NGo;
        p.Dmax = p.NG / 2;
        // waves (= consecutive row groups) per pair-kernel workgroup: their column-side partial accelerations are
        // combined in LDS, so the column slab holds one block per (workgroup, column tile) -- wg_waves times less
        // memory and traffic.  Only for 4-tile row groups with plenty of them.
        // Measured at n = 262144 (profiles/r02_wg_waves_lds_combine.txt): the lock step costs more than the smaller
        // slab saves -- pair kernel 18.0 / 18.8 / 19.9 ms, slab reduction 0.61 / 0.39 / 0.28 ms for 1 / 2 / 4 --
        // so the default stays 1 and a larger value is chosen only where the column slab would not fit a budget
        // (LJMD_SLAB_BUDGET_GB, default 64 of the card's 288 GB: n = 1 048 576 on ONE GPU keeps W = 1 with a 52 GB slab --
        // pair + reduction 287 ms against 303 ms with W = 4 and 13 GB -- and 2 097 152 particles run with W = 4, 52 GB).
        int wg = k.n3_wg_waves;
        if (wg != 1 && wg != 2 && wg != 4) {
            const double budget = 1e9 * k.slab_budget_gb;
            const double full = (double)p.T * (n_ranks > 1 ? p.NGo : p.Dmax + 1) * 3.0 * kTile * sizeof(double);   // slab_j at wg = 1
            wg = full <= budget ? 1 : full <= 2.0 * budget ? 2 : 4;
        }
        if (rt != kRowTiles || p.NGo < 16 * wg) wg = 1;
        p.wg_waves = wg;
        // the tie d = NG / 2 worked from both sides (N3Args::both_ties): equal work for every row group where there are few
        // of them; one rank, one wave per workgroup, fp64 mode
        p.both_ties = wg == 1 && n_ranks == 1 && !mixed_mode && p.NG <= kBothTiesMaxGroups && k.n3_both_ties;
        // slab_j: the blocks of a column tile lie together (N3Args::slab_j)
        p.j_by_group = (n_ranks > 1 || p.NG % wg != 0) ? 1 : 0;
        p.CS = p.j_by_group ? (p.NGo + wg - 1) / wg : (p.Dmax + wg - 1) / wg + 1;
        p.CS2 = n_ranks > 1 ? p.NGo : p.Dmax + 1;              // far pass: one wave per workgroup
        // (rc within 1e-9 of L/2 -- the reference accepts rc_over_L up to 0.5 and rejects only rc >= L/2 -- takes the exact
        //  generic kernel, which has no Newton-3 form: a multi-rank run then needs no force exchange at all, and every
        //  rank must know that when it allocates)
        p.use_n3 = k.n3 && n >= k.n3_min_n && (n_ranks == 1 || p.rc_allows_fast) &&
                   precision_mode != LJMD_PRECISION_FP64_REPRODUCIBLE;   // (the fixed-point kernel is a gather kernel)
        // work items = (row group, slice of its units), N3Args::uchunk.  Large systems: slices of whole offsets (dchunk),
        // ~target_waves items; a system with fewer (row group, offset) pairs than that is cut finer, down to one pass per item.
        const int n_off = p.Dmax + p.wg_waves;          // offsets a workgroup walks (relative to its first row group)
        const int n_units = n_off * rt;
        // (a rank of a multi-rank run always aims at 131 072: its kernel is 1 / G of a large system's, measured best with the
        //  most items -- profiles/r02_per_rank_xcd_threshold_and_target_waves.txt, r04_per_rank_work_items.txt)
        const bool plenty = (long)p.NGo * n_off >= kN3LargeItems || n_ranks > 1;
        const int target_waves = std::max(1, k.n3_target_waves.value_or(plenty ? 131072 : kN3MidTargetItems));
        const int ns_wanted = (target_waves + p.NGo - 1) / p.NGo;
        int ns = std::max(1, std::min(ns_wanted, n_off));
        // small single-rank systems: at most kDirectFoldMax work items, so that the step record is folded by ONE block
        // whichever way the step is launched (the fused step kernel keeps finalize_body's summation order, not fold_partials')
        const bool small_single = n_ranks == 1 && n <= kFuseTailMaxN && rt <= kFuseTailMaxRowTiles;
        const int ns_cap = small_single ? std::max(1, kDirectFoldMax / std::max(1, p.NGo)) : n_units;
        ns = std::min(ns, ns_cap);
        p.dchunk = (n_off + ns - 1) / ns;
        p.uchunk = p.dchunk * rt;
        if (!mixed_mode && ns_wanted > n_off) {                          // finer than whole offsets
            const int nsu = std::max(1, std::min(std::min(ns_wanted, ns_cap), n_units));
            p.uchunk = (n_units + nsu - 1) / nsu;
        }
        p.nslab_n = (n_units + p.uchunk - 1) / p.uchunk;
    }
    // two launches per step for small single-rank systems (tile_tail_kernel; ljmd_engine.h: fuse_tail)
    p.fuse_tail = k.fuse && k.fuse_tail && n_ranks == 1 && n <= kFuseTailMaxN && p.rc_allows_fast &&
                  precision_mode == LJMD_PRECISION_FP64 && (!p.use_n3 || (p.rt <= kFuseTailMaxRowTiles && p.wg_waves == 1));
    // the pair kernel's slices in two launches, most of the slab reduction beside the second (LaunchPlan::split_s1): one rank,
    // fp64, 4-tile row groups, one wave per workgroup, blocks numbered by offset.  The first launch must end on a whole offset
    // -- split_s1 * uchunk a multiple of rt -- so that it completes the blocks j < split_j1 of every column tile.
    if (n_ranks == 1 && precision_mode == LJMD_PRECISION_FP64 && p.use_n3 && p.rc_allows_fast && !p.fuse_tail &&
        p.rt == kRowTiles && p.wg_waves == 1 && !p.j_by_group && !k.force_collectives) {
        const int S = p.nslab_n;
        const int m = rt_align(p.uchunk, p.rt);                               // slices per whole number of offsets
        const int deferred = k.reduce_split.value_or(n >= kReduceSplitMinN ? (S + kReduceSplitShare - 1) / kReduceSplitShare : 0);
        if (deferred >= 1 && m < S) {
            const int s1 = std::max(m, (std::max(0, S - deferred) / m) * m);
            p.split_s1 = s1;
            p.split_j1 = s1 * p.uchunk / p.rt;
        }
    }
    const bool mixed = precision_mode == LJMD_PRECISION_FP32_FORCE;
    if (mixed && (!p.use_n3 || n < kMixedMinN))
        // the fp32 far kernel works on 4-tile row groups and only pays where most pairs are far pairs
        return fail(nullptr, LJMD_ERR_INVALID_ARG,
                    "ljmd_create: LJMD_PRECISION_FP32_FORCE needs the Newton-3 path and n >= %d", kMixedMinN);
    p.nslab_max = std::max(std::max(p.nslab_g, p.nslab_t), p.use_n3 ? p.nslab_n * (mixed ? 2 : 1) : 1);
    p.n_wg_max = std::max(row_blocks * std::max(p.nslab_g, p.nslab_t),
                          (p.NGo + 4) * p.nslab_n * (mixed ? 2 : 1));
    p.n_ke = row_blocks;
    *out = std::move(p);
    return LJMD_OK;
}

}  // namespace ljmdh
