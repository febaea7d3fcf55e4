// ljmd_migrate.cpp -- ownership migration of a sharded engine: pack | (exchange by the caller) | deal | rebase, and the
// ljmd_migrate* entry points of the C ABI.
#include "ljmd_engine.h"
#include "ljmd_multi.h"

namespace ljmdh {

namespace {
int migrate_prepare(ljmd_t *h)
{
    if (h->d_mig) return LJMD_OK;
    const size_t n = (size_t)h->n;
    // levels of the deal: segments = runs of whole shards, halved (lower half = ceil) until every segment is one shard.
    // LJMD_MIGRATE_DEAL=slabs (default): every level splits along x -- G slabs.  With rc ~ L/2 every rank needs every
    // position whatever the shape, so a compact surface buys nothing, while slabs are translation-symmetric in the
    // periodic box: the pair kernel's ownership rule (row group A owns the groups up to half the ring ahead) then gives
    // every rank the same work.  =blocks: the longest remaining extent (2 x 2 x 2 near-cubic blocks at G = 8) -- same total
    // work, but a rank's partners ahead on the ring are face, edge or corner neighbours depending on the rank: measured
    // 2.50 / 2.28 / 2.05 / 1.85 ms per rank (max / mean = 1.16) against 2.14-2.18 for slabs at n = 262144
    // (profiles/r03_deal_shapes_per_rank.txt).
    const bool blocks = h->knobs.migrate_blocks;
    std::vector<int> offsets, bounds = {0, h->G};
    double ext[3] = {h->L, h->L, h->L};
    while (true) {
        bool any = false;
        for (size_t j = 0; j + 1 < bounds.size(); ++j) any = any || (bounds[j + 1] - bounds[j] > 1);
        if (!any) break;
        h->mig_level_off.push_back(offsets.size());
        h->mig_level_nseg.push_back((int)bounds.size() - 1);
        for (int b : bounds) offsets.push_back(b * h->plan.S);
        int best = 0;
        if (blocks)
            for (int ax = 1; ax < 3; ++ax)
                if (ext[ax] > ext[best] * (1.0 + 1e-9)) best = ax;
        h->mig_axis.push_back(best);
        ext[best] *= 0.5;
        std::vector<int> next;
        for (size_t j = 0; j + 1 < bounds.size(); ++j) {
            next.push_back(bounds[j]);
            const int t = bounds[j + 1] - bounds[j];
            if (t > 1) next.push_back(bounds[j] + (t + 1) / 2);
        }
        next.push_back(h->G);
        bounds.swap(next);
    }
    for (int ax = 0; ax < 3; ++ax) h->mig_ext[ax] = ext[ax];
    LJMD_HIP(h, hipMalloc(&h->d_mig_idx, n * sizeof(int)));
    LJMD_HIP(h, hipMalloc(&h->d_mig_idx2, n * sizeof(int)));
    LJMD_HIP(h, hipMalloc(&h->d_mig_keys, n * sizeof(unsigned long long)));
    LJMD_HIP(h, hipMalloc(&h->d_mig_keys2, n * sizeof(unsigned long long)));
    h->mig_cub_bytes = kd_temp_bytes(h->n);
    LJMD_HIP(h, hipMalloc(&h->d_mig_cub, std::max<size_t>(h->mig_cub_bytes, 16)));
    LJMD_HIP(h, hipMalloc(&h->d_mig_offsets, std::max<size_t>(offsets.size(), 2) * sizeof(int)));
    if (!offsets.empty())
        LJMD_HIP(h, hipMemcpyAsync(h->d_mig_offsets, offsets.data(), offsets.size() * sizeof(int), hipMemcpyHostToDevice,
                                   h->stream));
    LJMD_HIP(h, hipStreamSynchronize(h->stream));      // `offsets` goes out of scope
    LJMD_HIP(h, hipMalloc(&h->d_mig, (size_t)h->G * kMigrateRows * h->plan.P * sizeof(double)));   // last: marks "prepared"
    return LJMD_OK;
}
}  // namespace

double *migrate_buffer(ljmd_t *h) { return h->d_mig; }

int migrate_pack(ljmd_t *h)
{
    const int rc_ = migrate_prepare(h);
    if (rc_ != LJMD_OK) return rc_;
    LJMD_HIP(h, launch_migrate_pack(h->d_ru, h->d_v, h->d_a, h->d_perm, h->d_gid0,
                                    h->d_mig + (size_t)h->rank * kMigrateRows * h->plan.P, h->plan.S, h->plan.P, h->stream));
    return LJMD_OK;
}

int migrate_deal(ljmd_t *h)
{
    if (!h->d_mig) return fail(h, LJMD_ERR_STATE, "migrate_deal: migrate_pack has not run");
    LJMD_HIP(h, launch_iota_blocked(h->d_mig_idx, h->n, h->plan.S, h->plan.P, h->stream));
    int *cur = h->d_mig_idx, *nxt = h->d_mig_idx2;
    for (size_t l = 0; l < h->mig_level_nseg.size(); ++l) {
        LJMD_HIP(h, kd_level_blocked(h->d_mig_cub, h->mig_cub_bytes, h->d_pos, h->mig_axis[l], h->plan.P, h->L, h->d_mig_keys,
                                     h->d_mig_keys2, cur, nxt, h->n, h->mig_level_nseg[l],
                                     h->d_mig_offsets + h->mig_level_off[l], h->stream));
        std::swap(cur, nxt);
    }
    LJMD_HIP(h, launch_migrate_select(h->d_pos, h->d_mig, cur + (size_t)h->rank * h->plan.S, h->d_tmp3, h->d_ru, h->d_v, h->d_a,
                                      h->d_gid0, h->plan.S, h->plan.P, h->stream));
    LJMD_HIP(h, hipMemcpyAsync(own_block(h), h->d_tmp3, 3 * (size_t)h->plan.P * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    // the new members in the order of the deal ARE the engine's original order now: identity permutation, then the
    // shard's own k-d order (split axes from the block's extents, as ljmd_set_state chooses them)
    LJMD_HIP(h, launch_iota(h->d_perm, h->plan.P, h->stream));
    for (int i = 0; i < h->plan.P; ++i) h->h_perm[i] = i;
    h->perm_dirty = false;
    {
        double ext[3] = {h->mig_ext[0], h->mig_ext[1], h->mig_ext[2]};
        h->kd_axis.assign(h->plan.kd_level_nseg.size(), 0);
        for (size_t l = 0; l < h->kd_axis.size(); ++l) {
            int best = 0;
            for (int ax = 1; ax < 3; ++ax)
                if (ext[ax] > ext[best] * (1.0 + 1e-9)) best = ax;
            h->kd_axis[l] = best;
            ext[best] *= 0.5;
        }
    }
    h->boxes_valid = false;
    h->h_gid0.resize(h->plan.P);
    LJMD_HIP(h, hipMemcpyAsync(h->h_gid0.data(), h->d_gid0, (size_t)h->plan.P * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    if (h->plan.sort_enabled && fast_path_ok(h)) {
        const int rc_ = resort(h, true);               // a(t) is live between two steps
        if (rc_ != LJMD_OK) return rc_;
    }
    LJMD_HIP(h, hipStreamSynchronize(h->stream));
    h->migrated = true;
    ++h->migrations;
    return LJMD_OK;
}

int migrate_rebase(ljmd_t *h)
{
    LJMD_HIP(h, launch_iota_offset(h->d_gid0, h->plan.S, h->plan.P, h->rank * h->plan.S, h->stream));
    h->migrated = false;
    return LJMD_OK;
}

}  // namespace ljmdh

extern "C" {

// ---- ownership migration (multi-GPU) -------------------------------------------------------------------------------

int ljmd_migrate_pack(ljmd_t *h)
{
    LJMD_TRY(entry_checks(h, "ljmd_migrate_pack", kHandle));
    if (h->multi) return fail(h, LJMD_ERR_STATE, "ljmd_migrate_pack: a multi-device handle migrates through ljmd_migrate");
    LJMD_TRY(entry_checks(h, "ljmd_migrate_pack", kHaveState));
    if (h->forces_pending) return fail(h, LJMD_ERR_STATE, "ljmd_migrate_pack: a step is half enqueued");
    LJMD_HIP(h, hipSetDevice(h->device));
    return migrate_pack(h);
}

void *ljmd_migrate_buffer(ljmd_t *h, int64_t *n_total, int64_t *own_off, int64_t *own_cnt)
{
    if (!h || h->multi) return nullptr;
    const int64_t blk = (int64_t)kMigrateRows * h->plan.P;
    if (n_total) *n_total = blk * h->G;
    if (own_off) *own_off = blk * h->rank;
    if (own_cnt) *own_cnt = blk;
    return migrate_buffer(h);
}

int ljmd_migrate_deal(ljmd_t *h)
{
    LJMD_TRY(entry_checks(h, "ljmd_migrate_deal", kHandle));
    if (h->multi) return fail(h, LJMD_ERR_STATE, "ljmd_migrate_deal: a multi-device handle migrates through ljmd_migrate");
    LJMD_HIP(h, hipSetDevice(h->device));
    return migrate_deal(h);
}

int ljmd_migrate(ljmd_t *h)
{
    LJMD_TRY(entry_checks(h, "ljmd_migrate", kHandle | kNotPoisoned));
    if (h->multi) return ljmdm::migrate_now(h);
    if (h->G == 1) return LJMD_OK;                       // one rank owns everything
    if (!h->comm) return fail(h, LJMD_ERR_STATE, "ljmd_migrate: no communicator (use ljmd_migrate_pack / _deal around your own exchange)");
    int rc_ = ljmd_migrate_pack(h);
    if (rc_ != LJMD_OK) return rc_;
    // all collectives of the communicator on ONE stream (see comm_begin): the blocks of everybody's ru, v, a and ids
    const bool cs = use_comm_stream(h);
    const hipStream_t xs = cs ? h->comm_stream : h->stream;
    if (cs && (rc_ = comm_begin(h)) != LJMD_OK) return rc_;
    const size_t blk = (size_t)kMigrateRows * h->plan.P;
    const ncclResult_t r = ncclAllGather(h->d_mig + (size_t)h->rank * blk, h->d_mig, blk, ncclDouble, h->comm, xs);
    if (r != ncclSuccess) return fail(h, LJMD_ERR_HIP, "ncclAllGather (migration) failed: %s", ncclGetErrorString(r));
    if (cs && (rc_ = comm_end(h)) != LJMD_OK) return rc_;
    if ((rc_ = migrate_deal(h)) != LJMD_OK) return rc_;
    h->gather_done_for_step = false;
    return ljmd_allgather_positions(h);                  // every rank's block changed
}

int ljmd_particle_ids(ljmd_t *h, int32_t *ids)
{
    if (!h || !ids) return fail(h, LJMD_ERR_INVALID_ARG, "ljmd_particle_ids: NULL argument");
    if (h->multi) {                                      // global arrays in the caller's order, whatever migrated inside
        for (int32_t k = 0; k < h->n; ++k) ids[k] = k;
        return LJMD_OK;
    }
    if (!h->migrated) {
        for (int32_t j = 0; j < h->plan.S; ++j) ids[j] = h->rank * h->plan.S + j;
        return LJMD_OK;
    }
    static_assert(sizeof(int32_t) == sizeof(int), "particle ids are int32");
    std::memcpy(ids, h->h_gid0.data(), (size_t)h->plan.S * sizeof(int32_t));
    return LJMD_OK;
}

}  // extern "C"
