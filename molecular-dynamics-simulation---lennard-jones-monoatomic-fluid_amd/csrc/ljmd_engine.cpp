// ljmd_engine.cpp -- the step phases of one engine: kernel argument builders, spatial re-sort, the communication-stream
// fences, drift | pair forces | kick on the engine's HIP stream, and the read-back of the per-step record ring.
#include "ljmd_engine.h"

namespace ljmdh {

bool fast_path_ok(const ljmd_t *h) { return h->plan.rc_allows_fast && h->positions_compact && !h->knobs.force_generic; }

// the buffer of workgroup partials of the current force evaluation (two of them alternate when the record of a step is
// folded by the next step's tail launch)
double *wg_part_now(ljmd_t *h) { return h->d_wg_part + (h->plan.fuse_tail ? (size_t)h->fold_parity * h->wg_part_stride : 0); }

PairArgs pair_args(ljmd_t *h, bool fast)
{
    PairArgs a;
    a.pos = h->d_pos;
    a.slab = h->d_slab;
    a.wg_part = wg_part_now(h);
    a.mask = h->d_mask;
    a.bbox = h->d_bbox;
    a.inline_mask = (fast && h->plan.fuse_tail && !h->plan.use_n3) ? 1 : 0;
    a.rc2_skin = h->rc2 * (1.0 + 1e-10);
    a.n = h->n;
    a.S = h->plan.S;
    a.P = h->plan.P;
    a.G = h->G;
    a.rank = h->rank;
    a.TB = h->plan.TB;
    a.T = h->plan.T;
    a.W = h->plan.W;
    a.chunk = fast ? h->plan.chunk_t : h->plan.chunk_g;
    a.L = h->L;
    a.invL = h->invL;
    a.rc2 = h->rc2;
    return a;
}

GeometryArgs geometry_args(ljmd_t *h)
{
    GeometryArgs a;
    a.pos = h->d_pos;
    a.bbox = h->d_bbox;
    a.pos_tc = h->plan.use_n3 ? h->d_pos_tc : nullptr;
    a.wrap_first = h->positions_wide ? 1 : 0;
    a.invL = h->invL;
    a.mask = h->d_mask;
    a.P = h->plan.P;
    a.G = h->G;
    a.rank = h->rank;
    a.TB = h->plan.TB;
    a.T = h->plan.T;
    a.W = h->plan.W;
    a.RT = h->plan.rt;
    a.L = h->L;
    a.rc2_skin = h->rc2 * (1.0 + 1e-10);
    a.mask_far = h->d_mask_far;       // NULL unless mixed precision
    a.rsplit2 = h->knobs.fp32_split * h->knobs.fp32_split;
    // 2^(26/3) = 406.3747: r^-6 < 2^-26 beyond it, 406.5 with a margin of 1e-3 for the fp32 roundings of u^3 (pair_n3_f32<., VFAR>);
    // LJMD_FP32_VFAR=0 switches the form off
    a.rvfar2 = h->knobs.fp32_vfar ? 406.5 : HUGE_VAL;
    a.pertile_images = h->knobs.n3_pertile ? 1 : 0;
    a.both_ties = h->plan.both_ties ? 1 : 0;
    return a;
}

N3Args n3_args(ljmd_t *h)
{
    N3Args a;
    a.pos = h->d_pos_tc;       // every tile in one periodic image (tile_boxes_kernel / the drift kernel's fused form)
    a.mask = h->d_mask;
    a.bbox = h->d_bbox;
    a.desc = h->d_desc;
    a.desc2 = h->d_desc2;
    a.slab_i = h->d_slab;
    a.slab_j = h->d_slab_j;
    a.flag_j = h->d_flag_j;
    a.wg_part = wg_part_now(h);
    a.S = h->plan.S;
    a.P = h->plan.P;
    a.G = h->G;
    a.rank = h->rank;
    a.TB = h->plan.TB;
    a.T = h->plan.T;
    a.W = h->plan.W;
    a.NG = h->plan.NG;
    a.NGo = h->plan.NGo;
    a.Dmax = h->plan.Dmax;
    a.CS = h->plan.CS;
    a.by_group = h->plan.j_by_group;
    a.dchunk = h->plan.dchunk;
    a.uchunk = h->plan.uchunk;
    a.by0 = 0;
    a.xcd_remap = 0;
    a.inline_class = (h->plan.fuse_tail && h->plan.rt <= 2 && h->plan.wg_waves == 1) ? 1 : 0;
    a.both_ties = h->plan.both_ties ? 1 : 0;
    a.rc2_skin = h->rc2 * (1.0 + 1e-10);
    a.energy = h->want_energy ? 1 : 0;
    a.RT = h->plan.rt;
    a.L = h->L;
    a.invL = h->invL;
    a.rc2 = h->rc2;
    return a;
}

IntegrateArgs integrate_args(ljmd_t *h)
{
    IntegrateArgs a;
    a.r = own_block(h);
    a.ru = h->d_ru;
    a.v = h->d_v;
    a.a = h->d_a;
    a.fsum = needs_force_exchange(h) ? h->d_frecv : h->d_fpart;
    a.bbox = nullptr;
    a.pos_tc = nullptr;
    a.RT = std::max(1, h->plan.rt);
    a.ticket = nullptr;
    a.ke_part = h->d_ke_part;
    a.rows = h->plan.P;
    a.P = h->plan.P;
    a.L = h->L;
    a.invL = h->invL;
    a.dt = h->dt;
    a.dt_half = h->dt_half;
    a.dt_sq_half = h->dt_sq_half;
    return a;
}

ReduceArgs reduce_args(ljmd_t *h, int nslab, bool n3)
{
    ReduceArgs a;
    a.slab = h->d_slab;
    a.slab_j = n3 ? h->d_slab_j : nullptr;
    a.flag_j = n3 ? h->d_flag_j : nullptr;
    a.slab_j2 = (n3 && h->mode == LJMD_PRECISION_FP32_FORCE) ? reinterpret_cast<const float *>(h->d_slab_j2) : nullptr;
    a.flag_j2 = (n3 && h->mode == LJMD_PRECISION_FP32_FORCE) ? h->d_flag_j2 : nullptr;
    a.fpart = h->d_fpart;
    a.nslab = nslab;
    a.P = h->plan.P;
    a.G = h->G;
    a.rank = h->rank;
    a.TB = h->plan.TB;
    a.CS = h->plan.CS;
    a.CS2 = h->plan.CS2;
    a.RT = h->plan.rt;
    a.partial = h->d_red_part;
    a.c_split = h->plan.split_s1;
    a.j_split = h->plan.split_j1;
    return a;
}

FinalizeArgs finalize_args(ljmd_t *h, int n_wg, bool with_ke, double pair_scale)
{
    FinalizeArgs a;
    a.pair_scale = pair_scale;
    a.wg_part = wg_part_now(h);
    a.ke_part = h->d_ke_part;
    a.ke_tile = nullptr;
    a.ring = h->d_ring;
    a.ring_pos = h->d_ring_pos;
    a.n_wg = n_wg;
    a.n_ke = with_ke ? h->plan.n_ke : 0;
    a.ring_cap = kRingCap;
    return a;
}

EventSet *next_events(ljmd_t *h)
{
    if (!h->profiling || h->ev_used >= (size_t)kMaxProfiledLaunches) return nullptr;
    if (h->ev_used == h->ev_pool.size()) {
        EventSet q;
        for (auto &e : q.e)
            if (hipEventCreate(&e) != hipSuccess) return nullptr;
        h->ev_pool.push_back(q);
    }
    EventSet *q = &h->ev_pool[h->ev_used++];
    q->has_pos_x = q->has_force_x = false;
    return q;
}

// Spatial re-ordering of the owned shard: keys -> stable sort -> gather r, ru, v (+ a when
// asked) and compose the slot->original permutation.  Performance only (ljmd_sort.hip).
int resort(ljmd_t *h, bool with_accel)
{
    if (!launch_kd_finish || !launch_gather_state)
        return fail(h, LJMD_ERR_HIP, "resort: this build holds no launch_kd_finish / launch_gather_state (ljmd_sort.h)");
    // recursive median split (ljmd_sort.hip) along the axis chosen for each level at set_state (longest remaining extent
    // of the shard): one composite-key radix sort of the whole shard per level while a segment is larger than a workgroup
    // of kd_finish_kernel sorts, then every remaining level in that kernel
    const int levels = (int)h->plan.kd_level_nseg.size(), from = h->plan.kd_finish_from;
    int *cur = h->d_idx, *nxt = h->d_idx2;
    LJMD_HIP(h, launch_iota(cur, h->plan.P, h->stream));
    if (from > 0) LJMD_HIP(h, launch_iota(nxt, h->plan.P, h->stream));   // slots S..P-1 (padding) keep their identity in both
    for (int l = 0; l < from; ++l) {
        const double *axis = own_block(h) + (size_t)h->kd_axis[l] * h->plan.P;
        LJMD_HIP(h, kd_level(h->d_cub, h->cub_bytes, axis, h->L, h->d_kd_keys, h->d_kd_keys2, cur, nxt, h->plan.S,
                             h->plan.kd_level_nseg[l], h->d_kd_offsets + h->plan.kd_level_off[l], h->stream));
        std::swap(cur, nxt);
    }
    for (int l = from; l < levels; l += kKdFinishMaxLevels) {            // (one launch: 64 tiles halve to one in 6 levels)
        KdFinishArgs ka;
        ka.pos = own_block(h);
        ka.P = h->plan.P;
        ka.scale = (double)(1u << kCoordBits) / h->L;
        ka.idx_in = ka.idx_out = cur;
        ka.offsets = h->d_kd_offsets;
        ka.nlevels = std::min(kKdFinishMaxLevels, levels - l);
        for (int k = 0; k < ka.nlevels; ++k) {
            ka.nseg[k] = h->plan.kd_level_nseg[l + k];
            ka.off[k] = (int)h->plan.kd_level_off[l + k];
            ka.axis[k] = h->kd_axis[l + k];
        }
        LJMD_HIP(h, launch_kd_finish(ka, h->stream));
    }
    // everything that follows the permutation in one launch; ru, v, a trade places with their scratch sets, the positions
    // go back into the exchange buffer, whose block is not the engine's to move
    GatherStateArgs g;
    double *sets[4] = {own_block(h), h->d_ru, h->d_v, with_accel ? h->d_a : nullptr};
    double *outs[4] = {h->d_tmp3, h->d_ru2, h->d_v2, h->d_a2};
    for (int k = 0; k < 4; ++k) {
        g.src[k] = sets[k];
        g.dst[k] = outs[k];
    }
    g.perm = h->d_perm;
    g.perm_out = h->d_perm2;
    g.idx = cur;
    g.P = h->plan.P;
    LJMD_HIP(h, launch_gather_state(g, h->stream));
    LJMD_HIP(h, hipMemcpyAsync(own_block(h), h->d_tmp3, 3 * (size_t)h->plan.P * sizeof(double), hipMemcpyDeviceToDevice,
                               h->stream));
    std::swap(h->d_ru, h->d_ru2);
    std::swap(h->d_v, h->d_v2);
    if (with_accel) std::swap(h->d_a, h->d_a2);
    std::swap(h->d_perm, h->d_perm2);
    h->perm_dirty = true;
    h->steps_since_sort = 0;
    return LJMD_OK;
}

int refresh_perm(ljmd_t *h)
{
    if (!h->perm_dirty) return LJMD_OK;
    LJMD_HIP(h, hipMemcpyAsync(h->h_perm.data(), h->d_perm, (size_t)h->plan.P * sizeof(int), hipMemcpyDeviceToHost,
                               h->stream));
    LJMD_HIP(h, hipStreamSynchronize(h->stream));
    h->perm_dirty = false;
    return LJMD_OK;
}

// All collectives of the communicator go through ONE stream.  With the communication stream in use
// (LJMD_OVERLAP_EXCHANGE=1, default) a collective is fenced against the engine's stream by two events:
// comm_begin = "the engine's work so far is a prerequisite", comm_end = "the engine's later work waits for it".
bool use_comm_stream(const ljmd_t *h) { return h->knobs.overlap_exchange && h->comm_stream != nullptr; }

int comm_begin(ljmd_t *h)
{
    LJMD_HIP(h, hipEventRecord(h->ev_pos_ready, h->stream));
    LJMD_HIP(h, hipStreamWaitEvent(h->comm_stream, h->ev_pos_ready, 0));
    return LJMD_OK;
}

int comm_end(ljmd_t *h)
{
    LJMD_HIP(h, hipEventRecord(h->ev_gather_done, h->comm_stream));
    LJMD_HIP(h, hipStreamWaitEvent(h->stream, h->ev_gather_done, 0));
    return LJMD_OK;
}

int allgather_on(ljmd_t *h, hipStream_t s)
{
    // in place: the send block is this rank's slice of the receive buffer
    const ncclResult_t r = ncclAllGather(own_block(h), h->d_pos, 3 * (size_t)h->plan.P, ncclDouble, h->comm, s);
    if (r != ncclSuccess) return fail(h, LJMD_ERR_HIP, "ncclAllGather failed: %s", ncclGetErrorString(r));
    return LJMD_OK;
}

// Phase A: pair kernel on the exchange buffer + deterministic slab reduction into fpart.
int enqueue_pair_forces(ljmd_t *h, EventSet *q)
{
    if (h->inject_failure_at >= 0 && (int)h->ring_issued == h->inject_failure_at) {
        h->inject_failure_at = -1;
        return fail(h, LJMD_ERR_HIP, "injected failure in the force phase (LJMD_INJECT_FAILURE_AT_STEP)");
    }
    const bool fast = fast_path_ok(h);
    if (q) LJMD_HIP(h, hipEventRecord(q->e[1], h->stream));
    if (reproducible(h)) {
        // exact fixed-point gather kernel: the tile-pair mask where the fast path's preconditions hold, every tile otherwise
        if (fast) {
            const GeometryArgs ga = geometry_args(h);
            if (!h->boxes_valid) LJMD_HIP(h, launch_tile_boxes(ga, h->stream));
            LJMD_HIP(h, launch_tile_mask(ga, h->stream));
        }
        h->boxes_valid = false;
        if (q) LJMD_HIP(h, hipEventRecord(q->e[2], h->stream));
        FixedArgs fa;
        fa.pos = h->d_pos;
        fa.mask = h->d_mask;
        fa.fslab = h->d_fslab;
        fa.fflag = h->d_fflag;
        fa.walk_all = fast ? 0 : 1;
        fa.S = h->plan.S; fa.P = h->plan.P; fa.G = h->G; fa.rank = h->rank; fa.TB = h->plan.TB; fa.T = h->plan.T; fa.W = h->plan.W;
        fa.chunk = h->plan.chunk_t;
        fa.energy = h->want_energy ? 1 : 0;
        fa.L = h->L; fa.invL = h->invL; fa.rc2 = h->rc2;
        LJMD_HIP(h, launch_pair_fixed(fa, dim3(h->plan.TB / kWavesPerBlock, h->plan.nslab_t), h->stream));
        if (q) LJMD_HIP(h, hipEventRecord(q->e[3], h->stream));
        h->pending_energy = h->want_energy;
        h->reduce_deferred = false;
        h->forces_pending = true;
        return LJMD_OK;
    }
    int nslab, n_wg;
    bool n3 = false;
    bool split = false;             // the slab reduction's first phase is already enqueued: the second one is left
    if (fast) {
        GeometryArgs ga = geometry_args(h);
        if (!h->plan.use_n3) ga.mask_far = nullptr;
        if (!h->boxes_valid) LJMD_HIP(h, launch_tile_boxes(ga, h->stream));
        h->boxes_valid = false;                    // good for this evaluation only
        if (h->plan.fuse_tail)
            ;               // small single-rank system: the pair kernel's waves work their pass descriptors / mask words out themselves
        else if (h->plan.use_n3)      // tile-pair test + pass descriptors of the Newton-3 kernels in one launch (mixed mode: NEAR and FAR)
            LJMD_HIP(h, launch_tile_class(ga, h->invL, h->rc2, h->plan.S, h->plan.NGo, h->d_desc,
                                          h->mode == LJMD_PRECISION_FP32_FORCE ? h->d_desc_far : nullptr, h->d_desc2, h->stream));
        else                // the gather kernel reads the bit mask
            LJMD_HIP(h, launch_tile_mask(ga, h->stream));
        if (q) LJMD_HIP(h, hipEventRecord(q->e[2], h->stream));
        if (h->plan.use_n3) {
            const dim3 grid((h->plan.NGo + h->plan.wg_waves - 1) / h->plan.wg_waves, h->plan.nslab_n);     // wg_waves row groups per workgroup
            N3Args na = n3_args(h);
            // (kXcdMinGroups = 256 row groups per rank: with 4096 column tiles and 256 row groups -- rank
            //  0 of 4 at n = 262144 -- the mapping still saves 4.7 % (tools/probe_rank.py), with 128 it is neutral, as it
            //  is for single-rank systems of 16384..65536 particles)
            na.xcd_remap = (h->knobs.xcd_remap > 0 && (int)grid.x >= kXcdMinGroups && grid.x % (8 * h->knobs.xcd_remap) == 0) ? h->knobs.xcd_remap : 0;
            // mixed precision: the two pair kernels write disjoint slabs and partials -- the far pass (the long one) goes to
            // its own stream first and the near pass, mostly descriptor look-ups with a few passes between them, runs beside it
            const bool far_beside = h->mode == LJMD_PRECISION_FP32_FORCE && h->far_stream != nullptr;
            split = h->plan.split_s1 > 0 && h->side_stream != nullptr;
            if (split) {
                // Two launches over disjoint slices (LaunchPlan::split_s1).  The second needs nothing of the first and goes to
                // the side stream, whose priority is the lowest: its workgroups fill the first launch's drain, and the first
                // phase of the slab reduction -- HBM-bound, over what the first launch completed -- runs beside it.  The
                // streams join before the second phase.
                const int s1 = h->plan.split_s1;
                LJMD_HIP(h, hipEventRecord(h->ev_side_go, h->stream));
                LJMD_HIP(h, hipStreamWaitEvent(h->side_stream, h->ev_side_go, 0));
                LJMD_HIP(h, launch_pair_n3(na, dim3(grid.x, s1), h->plan.wg_waves, h->stream));
                N3Args nb = na;
                nb.by0 = s1;
                LJMD_HIP(h, launch_pair_n3(nb, dim3(grid.x, grid.y - s1), h->plan.wg_waves, h->side_stream));
                LJMD_HIP(h, launch_reduce_forces_split(reduce_args(h, h->plan.nslab_n, true), 1, h->stream));
                LJMD_HIP(h, hipEventRecord(h->ev_side_done, h->side_stream));
                LJMD_HIP(h, hipStreamWaitEvent(h->stream, h->ev_side_done, 0));
            } else if (far_beside) {
                LJMD_HIP(h, hipEventRecord(h->ev_far_go, h->stream));
                LJMD_HIP(h, hipStreamWaitEvent(h->far_stream, h->ev_far_go, 0));
            } else {
                LJMD_HIP(h, launch_pair_n3(na, grid, h->plan.wg_waves, h->stream));        // all pairs, or the NEAR ones
            }
            nslab = h->plan.nslab_n;
            n_wg = grid.x * grid.y * h->plan.wg_waves;                                      // one partial per wave
            n3 = true;
            if (h->mode == LJMD_PRECISION_FP32_FORCE) {
                const dim3 fgrid(h->plan.NGo, h->plan.nslab_n);                                  // one wave per workgroup
                // far pass in fp32: its own row-side slices, column-side slab and workgroup partials
                N3Args fa = n3_args(h);
                fa.mask = h->d_mask_far;
                fa.slab_i = h->d_slab + (size_t)h->plan.nslab_n * 3 * h->plan.P;
                fa.slab_j = h->d_slab_j2;
                fa.flag_j = h->d_flag_j2;
                fa.desc = h->d_desc_far;
                fa.CS = h->plan.CS2;
                fa.by_group = h->G > 1 ? 1 : 0;          // one wave per workgroup whatever wg_waves is: block index = offset d
                                                         // (CS2 = Dmax + 1) on one rank, the row group on several (CS2 = NGo)
                fa.xcd_remap = (h->knobs.xcd_remap > 0 && (int)fgrid.x >= kXcdMinGroups && fgrid.x % (8 * h->knobs.xcd_remap) == 0) ? h->knobs.xcd_remap : 0;
                fa.wg_part = h->d_wg_part + 2 * (size_t)n_wg;
                LJMD_HIP(h, launch_pair_n3_f32(fa, fgrid, far_beside ? h->far_stream : h->stream));
                if (far_beside) {
                    LJMD_HIP(h, hipEventRecord(h->ev_far_done, h->far_stream));
                    LJMD_HIP(h, launch_pair_n3(na, grid, h->plan.wg_waves, h->stream));    // the NEAR pairs, beside the far pass
                    LJMD_HIP(h, hipStreamWaitEvent(h->stream, h->ev_far_done, 0));
                }
                nslab *= 2;
                n_wg += fgrid.x * fgrid.y;
            }
        } else {
            const dim3 grid(h->plan.TB / kWavesPerBlock, h->plan.nslab_t);
            LJMD_HIP(h, launch_pair_tiles(pair_args(h, true), grid, h->stream));
            nslab = h->plan.nslab_t;
            n_wg = grid.x * grid.y;
        }
    } else {
        if (h->plan.use_n3 && h->G > 1)
            return fail(h, LJMD_ERR_STATE,
                        "multi-rank Newton-3 run needs wrapped positions and rc <= (1-1e-9) L/2 (set LJMD_N3=0)");
        if (q) LJMD_HIP(h, hipEventRecord(q->e[2], h->stream));
        const dim3 grid(h->plan.P / kBlock, h->plan.nslab_g);
        LJMD_HIP(h, launch_pair_rows_generic(pair_args(h, false), grid, h->stream));
        nslab = h->plan.nslab_g;
        n_wg = grid.x * grid.y;
    }
    if (q) LJMD_HIP(h, hipEventRecord(q->e[3], h->stream));
    h->reduce_deferred = fast && h->plan.fuse_tail && h->kick_hint >= 0 && n_wg <= kDirectFoldMax && !needs_force_exchange(h);
    if (h->reduce_deferred) {            // the tail launch of enqueue_kick reduces, kicks and folds the record in one kernel
        h->deferred_nslab = nslab;
        h->deferred_n3 = n3;
    } else if (split) {
        LJMD_HIP(h, launch_reduce_forces_split(reduce_args(h, nslab, n3), 2, h->stream));
    } else {
        LJMD_HIP(h, launch_reduce_forces(reduce_args(h, nslab, n3), needs_force_exchange(h), h->stream));
    }
    h->forces_pending = true;
    h->pending_n_wg = n_wg;
    h->pending_scale = n3 ? 1.0 : 0.5;
    return LJMD_OK;
}

// Phase B: (multi-rank Newton-3) reduce-scatter of the partial accelerations, then x24, optional
// second half-kick, kinetic-energy partials and this step's partial record.
int enqueue_kick(ljmd_t *h, bool kick, EventSet *q)
{
    if (reproducible(h)) {
        // integer sum of the slices, one rounding, x24, kick, exact per-block partials; then ONE record (no force exchange:
        // every rank owns its rows completely)
        FixedTailArgs ta;
        ta.fslab = h->d_fslab;
        ta.fflag = h->d_fflag;
        ta.nslab = h->plan.nslab_t;
        ta.P = h->plan.P;
        ta.TB = h->plan.TB;
        ta.a = h->d_a;
        ta.v = h->d_v;
        ta.dt_half = h->dt_half;
        ta.blk = h->d_fblk;
        LJMD_HIP(h, launch_fixed_tail(ta, kick, h->pending_energy, false, h->stream));
        FixedFoldArgs fo;
        fo.blk = h->d_fblk;
        fo.n_blk = h->plan.P / kBlock;
        fo.rec = reinterpret_cast<int64_t *>(h->d_ring);
        fo.ring_pos = h->d_ring_pos;
        fo.ring_cap = kRingCap;
        LJMD_HIP(h, launch_fixed_fold(fo, h->stream));
        if (q) LJMD_HIP(h, hipEventRecord(q->e[4], h->stream));
        h->ring_issued++;
        h->have_accel = true;
        h->forces_pending = false;
        return LJMD_OK;
    }
    if (h->reduce_deferred) {
        h->reduce_deferred = false;
        const bool drift = kick && h->next_drift_hint;
        IntegrateArgs ia = integrate_args(h);
        ia.ticket = h->d_ticket;
        if (drift) {                     // the next step's K1 writes the tile boxes and the coherent copy as well
            ia.bbox = h->d_bbox;
            ia.pos_tc = h->plan.use_n3 ? h->d_pos_tc : nullptr;
        }
        FinalizeArgs fa = finalize_args(h, h->pending_n_wg, kick, h->pending_scale);
        fa.ke_tile = h->d_ke_tile + (size_t)h->fold_parity * 3 * h->plan.T;
        // another step of this batch follows: its tail launch folds this step's record beside its own work
        const bool defer = kick && h->next_drift_hint && h->knobs.fuse_defer_record;
        FinalizeArgs prev{};
        if (h->fold_pending) prev = h->pending_fold;
        if (defer) ia.ticket = nullptr;
        LJMD_HIP(h, launch_tile_tail(reduce_args(h, h->deferred_nslab, h->deferred_n3), ia, fa, prev, kick, drift, h->stream));
        h->fold_pending = defer;
        h->pending_fold = fa;
        h->fold_parity ^= 1;                 // the next force evaluation writes the other pair of buffers
        if (q) LJMD_HIP(h, hipEventRecord(q->e[4], h->stream));
        h->drift_prefused = drift;
        h->ring_issued++;
        h->have_accel = true;
        h->forces_pending = false;
        return LJMD_OK;
    }
    if (needs_force_exchange(h) && !h->external_force_exchange) {
        if (!h->comm) return fail(h, LJMD_ERR_STATE, "multi-rank Newton-3 step: call ljmd_comm_init first");
        const bool cs = use_comm_stream(h);
        if (cs) {
            const int rc_ = comm_begin(h);
            if (rc_ != LJMD_OK) return rc_;
        }
        const hipStream_t xs = cs ? h->comm_stream : h->stream;
        const size_t blk = 3 * (size_t)h->plan.P;
        if (q) LJMD_HIP(h, hipEventRecord(q->e[7], xs));
        if (h->knobs.exchange_alltoall) {
            // every rank sends block g of its fpart straight to rank g (one xGMI link per peer on the fully
            // connected mesh) and adds the G blocks it receives in rank order: explicit, reproducible sum order
            ncclResult_t r = ncclGroupStart();
            for (int g = 0; g < h->G && r == ncclSuccess; ++g) {
                r = ncclSend(h->d_fpart + (size_t)g * blk, blk, ncclDouble, g, h->comm, xs);
                if (r == ncclSuccess) r = ncclRecv(h->d_fall + (size_t)g * blk, blk, ncclDouble, g, h->comm, xs);
            }
            const ncclResult_t e = ncclGroupEnd();
            if (r == ncclSuccess) r = e;
            if (r != ncclSuccess) return fail(h, LJMD_ERR_HIP, "force all-to-all failed: %s", ncclGetErrorString(r));
            LJMD_HIP(h, launch_sum_blocks(h->d_fall, h->d_frecv, h->G, (int)blk, xs));
        } else {
            const ncclResult_t r = ncclReduceScatter(h->d_fpart, h->d_frecv, blk, ncclDouble, ncclSum, h->comm, xs);
            if (r != ncclSuccess) return fail(h, LJMD_ERR_HIP, "ncclReduceScatter failed: %s", ncclGetErrorString(r));
        }
        if (q) {
            LJMD_HIP(h, hipEventRecord(q->e[8], xs));
            q->has_force_x = true;
        }
        if (cs) {
            const int rc_ = comm_end(h);
            if (rc_ != LJMD_OK) return rc_;
        }
    }
    if (h->fold_pending) {               // (a record left to "the next tail launch" that is not coming: append it now)
        LJMD_HIP(h, launch_finalize(h->pending_fold, nullptr, h->stream));
        h->fold_pending = false;
    }
    if (h->knobs.fuse && h->pending_n_wg <= kDirectFoldMax) {
        IntegrateArgs ia = integrate_args(h);
        ia.ticket = h->d_ticket;
        LJMD_HIP(h, launch_kick_finalize(ia, finalize_args(h, h->pending_n_wg, kick, h->pending_scale), kick, h->stream));
    } else {
        LJMD_HIP(h, launch_kick(integrate_args(h), kick, h->stream));
        LJMD_HIP(h, launch_finalize(finalize_args(h, h->pending_n_wg, kick, h->pending_scale), h->d_fold, h->stream));
    }
    if (q) LJMD_HIP(h, hipEventRecord(q->e[4], h->stream));
    h->ring_issued++;
    h->have_accel = true;
    h->forces_pending = false;
    return LJMD_OK;
}

int enqueue_forces(ljmd_t *h, bool kick, EventSet *q, bool next_drift)
{
    h->kick_hint = kick ? 1 : 0;         // both phases from one caller: the tail launch may take everything behind the pair kernel
    h->next_drift_hint = next_drift;
    int rc_ = enqueue_pair_forces(h, q);
    if (rc_ == LJMD_OK) rc_ = enqueue_kick(h, kick, q);
    h->kick_hint = -1;
    h->next_drift_hint = false;
    h->reduce_deferred = false;
    return rc_;
}

// K1, positions: drift + wrap + unwrapped update.  On a re-sort step (and only then) the whole of K1 runs here, followed
// by the re-sort: the velocity half-kick must precede the permutation, so there is nothing left to overlap (*split = false).
int enqueue_drift_positions(ljmd_t *h, EventSet *q, bool *split)
{
    if (q) LJMD_HIP(h, hipEventRecord(q->e[0], h->stream));
    h->gather_done_for_step = false;
    const bool resort_now = h->plan.sort_enabled && fast_path_ok(h) && h->steps_since_sort + 1 >= h->plan.resort_every;
    *split = !resort_now;
    LJMD_HIP(h, launch_drift_kick(integrate_args(h), resort_now ? 0 : 1, h->stream));
    h->positions_compact = true;  // freshly wrapped into [0, L]
    h->positions_wide = false;
    if (h->plan.sort_enabled && fast_path_ok(h) && ++h->steps_since_sort >= h->plan.resort_every) {
        if (*split) {             // (positions that only became compact with this wrap: finish K1 before permuting)
            LJMD_HIP(h, launch_drift_kick(integrate_args(h), 2, h->stream));
            *split = false;
        }
        return resort(h, false);  // a(t) is dead after the drift/kick: K3 rewrites it
    }
    return LJMD_OK;
}

// K1, velocities: the first half-kick (reads a(t), which nothing rewrites before the kick kernel of this step)
int enqueue_drift_velocities(ljmd_t *h)
{
    LJMD_HIP(h, launch_drift_kick(integrate_args(h), 2, h->stream));
    return LJMD_OK;
}

int enqueue_drift(ljmd_t *h, EventSet *q)
{
    const bool collectives = h->comm && (h->G > 1 || h->knobs.force_collectives);
    if (collectives && use_comm_stream(h)) {
        // positions first; the all-gather starts on the communication stream as soon as they are final and
        // overlaps the velocity half-kick; the engine's stream resumes (geometry pre-pass, pair kernel) when
        // the gathered positions have arrived.  (Re-sort steps permute the block after K1: the gather then follows
        // serially, ljmd_allgather_positions.)
        bool split = false;
        int rc_ = enqueue_drift_positions(h, q, &split);
        if (rc_ != LJMD_OK || !split) return rc_;
        rc_ = comm_begin(h);
        if (rc_ != LJMD_OK) return rc_;
        if (q) LJMD_HIP(h, hipEventRecord(q->e[5], h->comm_stream));
        rc_ = allgather_on(h, h->comm_stream);
        if (rc_ != LJMD_OK) return rc_;
        if (q) {
            LJMD_HIP(h, hipEventRecord(q->e[6], h->comm_stream));
            q->has_pos_x = true;
        }
        LJMD_HIP(h, hipEventRecord(h->ev_gather_done, h->comm_stream));
        rc_ = enqueue_drift_velocities(h);                                   // runs while the gather is in flight
        if (rc_ != LJMD_OK) return rc_;
        LJMD_HIP(h, hipStreamWaitEvent(h->stream, h->ev_gather_done, 0));
        h->gather_done_for_step = true;
        return LJMD_OK;
    }
    if (q) LJMD_HIP(h, hipEventRecord(q->e[0], h->stream));
    h->gather_done_for_step = false;
    const bool resort_now = h->plan.sort_enabled && fast_path_ok(h) && h->steps_since_sort + 1 >= h->plan.resort_every;
    if (h->drift_prefused) {
        // the previous step's tail launch has already run this K1 (tile_tail_kernel<.., DRIFT>), boxes included
        h->drift_prefused = false;
        h->boxes_valid = !resort_now && fast_path_ok(h);
        h->positions_compact = true;
        h->positions_wide = false;
        if (h->plan.sort_enabled && fast_path_ok(h) && ++h->steps_since_sort >= h->plan.resort_every) return resort(h, false);
        return LJMD_OK;
    }
    IntegrateArgs ia = integrate_args(h);
    // single rank, no re-sort behind this kernel: the drift kernel's waves are the tiles -- let them write
    // the bounding boxes of the new positions and skip tile_boxes_kernel in the force evaluation that follows
    // (only where a launch matters: at n = 262144 the six wave reductions cost the HBM-bound kernel more -- 8.0 ->
    // 11.5 us -- than the 5 us boxes kernel they replace)
    h->boxes_valid = h->knobs.fuse && h->G == 1 && h->n <= 65536 && !resort_now && fast_path_ok(h);
    if (h->boxes_valid) {
        ia.bbox = h->d_bbox;
        ia.pos_tc = h->plan.use_n3 ? h->d_pos_tc : nullptr;
    }
    LJMD_HIP(h, launch_drift_kick(ia, 0, h->stream));
    h->positions_compact = true;  // freshly wrapped into [0, L]
    h->positions_wide = false;
    if (h->plan.sort_enabled && fast_path_ok(h) && ++h->steps_since_sort >= h->plan.resort_every)
        return resort(h, false);  // a(t) is dead after the drift/kick: K3 rewrites it
    return LJMD_OK;
}

// Reads back the not-yet-consumed partial records (at most kRingCap) into h_ring.
int fetch_ring(ljmd_t *h, unsigned count)
{
    if (count > h->ring_issued - h->ring_consumed)
        return fail(h, LJMD_ERR_STATE, "requested %u step records but only %u are pending", count,
                    h->ring_issued - h->ring_consumed);
    h->ring_consumed = h->ring_issued - count;  // older unread records are dropped
    unsigned done = 0;
    while (done < count) {
        const unsigned pos = (h->ring_consumed + done) % kRingCap;
        const unsigned run = std::min(count - done, kRingCap - pos);
        LJMD_HIP(h, hipMemcpyAsync(h->h_ring + (size_t)done * h->rec_stride,
                                   h->d_ring + (size_t)pos * h->rec_stride,
                                   (size_t)run * h->rec_stride * sizeof(double),
                                   hipMemcpyDeviceToHost, h->stream));
        done += run;
    }
    LJMD_HIP(h, hipStreamSynchronize(h->stream));
    h->ring_consumed = h->ring_issued;
    return LJMD_OK;
}

}  // namespace ljmdh
