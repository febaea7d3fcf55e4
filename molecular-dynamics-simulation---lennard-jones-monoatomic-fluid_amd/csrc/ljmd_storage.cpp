// ljmd_storage.cpp -- what an engine owns: allocation and release of its device and pinned host memory, and the
// transfers of particle arrays between the caller's order and the device's slot order.
#include "ljmd_engine.h"

namespace ljmdh {

int allocate_engine(ljmd_t *h)
{
    const bool mixed = h->mode == LJMD_PRECISION_FP32_FORCE;
    const std::vector<int> &kd = h->plan.kd_offsets;
    LJMD_HIP(h, hipSetDevice(h->device));
    LJMD_HIP(h, hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    const size_t P3 = 3 * (size_t)h->plan.P * sizeof(double);
    LJMD_HIP(h, hipMalloc(&h->d_pos, P3 * h->G));
    LJMD_HIP(h, hipMalloc(&h->d_ru, P3));
    LJMD_HIP(h, hipMalloc(&h->d_v, P3));
    LJMD_HIP(h, hipMalloc(&h->d_a, P3));
    LJMD_HIP(h, hipMalloc(&h->d_tmp3, P3));
    if (h->plan.sort_enabled) {
        LJMD_HIP(h, hipMalloc(&h->d_ru2, P3));
        LJMD_HIP(h, hipMalloc(&h->d_v2, P3));
        LJMD_HIP(h, hipMalloc(&h->d_a2, P3));
    }
    LJMD_HIP(h, hipMalloc(&h->d_slab, P3 * h->plan.nslab_max));
    h->wg_part_stride = 2 * (size_t)h->plan.n_wg_max;
    LJMD_HIP(h, hipMalloc(&h->d_wg_part, (h->plan.fuse_tail ? 2 : 1) * h->wg_part_stride * sizeof(double)));
    if (h->plan.use_n3) {
        const size_t n_blk = (size_t)h->plan.T * h->plan.CS;
        LJMD_HIP(h, hipMalloc(&h->d_slab_j, n_blk * 3 * kTile * sizeof(double)));
        LJMD_HIP(h, hipMalloc(&h->d_flag_j, n_blk));
        LJMD_HIP(h, hipMemsetAsync(h->d_flag_j, 0, n_blk, h->stream));
        LJMD_HIP(h, hipMalloc(&h->d_desc, (size_t)h->plan.NGo * h->plan.T * sizeof(unsigned)));
        // cluster passes (ljmd_kernels.hip: n3_cluster_pass): 4-tile row groups, one wave per workgroup
        if (h->plan.rt == kRowTiles && h->plan.wg_waves == 1 && h->knobs.n3_clusters)
            LJMD_HIP(h, hipMalloc(&h->d_desc2, (size_t)h->plan.NGo * h->plan.T * 8 * sizeof(float)));
        LJMD_HIP(h, hipMalloc(&h->d_pos_tc, P3 * h->G));
    }
    if (h->plan.split_s1 > 0) {
        LJMD_HIP(h, hipMalloc(&h->d_red_part, (size_t)h->plan.TB * kWavesPerBlock * 3 * kTile * sizeof(double)));
        int least = 0, greatest = 0;       // numerically: least = the lowest priority
        LJMD_HIP(h, hipDeviceGetStreamPriorityRange(&least, &greatest));
        LJMD_HIP(h, hipStreamCreateWithPriority(&h->side_stream, hipStreamNonBlocking, least));
        LJMD_HIP(h, hipEventCreateWithFlags(&h->ev_side_go, hipEventDisableTiming));
        LJMD_HIP(h, hipEventCreateWithFlags(&h->ev_side_done, hipEventDisableTiming));
    }
    if (mixed && h->knobs.fp32_far_stream) {
        LJMD_HIP(h, hipStreamCreateWithFlags(&h->far_stream, hipStreamNonBlocking));
        LJMD_HIP(h, hipEventCreateWithFlags(&h->ev_far_go, hipEventDisableTiming));
        LJMD_HIP(h, hipEventCreateWithFlags(&h->ev_far_done, hipEventDisableTiming));
    }
    if (mixed) {
        LJMD_HIP(h, hipMalloc(&h->d_mask_far, (size_t)h->plan.TB * h->plan.W * sizeof(uint64_t)));
        LJMD_HIP(h, hipMalloc(&h->d_desc_far, (size_t)h->plan.NGo * h->plan.T * sizeof(unsigned)));
        const size_t n_blk2 = (size_t)h->plan.T * h->plan.CS2;
        LJMD_HIP(h, hipMalloc(&h->d_slab_j2, n_blk2 * 3 * kTile * sizeof(float)));     // fp32 blocks (pair_n3_f32_kernel)
        LJMD_HIP(h, hipMalloc(&h->d_flag_j2, n_blk2));
        LJMD_HIP(h, hipMemsetAsync(h->d_flag_j2, 0, n_blk2, h->stream));
    }
    LJMD_HIP(h, hipMalloc(&h->d_fpart, P3 * (needs_force_exchange(h) ? h->G : 1)));
    if (needs_force_exchange(h)) LJMD_HIP(h, hipMalloc(&h->d_frecv, P3));
    if (needs_force_exchange(h) && h->knobs.exchange_alltoall) LJMD_HIP(h, hipMalloc(&h->d_fall, P3 * h->G));
    LJMD_HIP(h, hipMalloc(&h->d_ke_part, 3 * (size_t)h->plan.n_ke * sizeof(double)));
    LJMD_HIP(h, hipMalloc(&h->d_fold, 2 * (size_t)kFoldBlocks * sizeof(double)));
    LJMD_HIP(h, hipMalloc(&h->d_ticket, sizeof(unsigned)));
    LJMD_HIP(h, hipMemsetAsync(h->d_ticket, 0, sizeof(unsigned), h->stream));
    if (h->plan.fuse_tail) {
        LJMD_HIP(h, hipMalloc(&h->d_ke_tile, 2 * 3 * (size_t)h->plan.T * sizeof(double)));        // two buffers, as wg_part
        LJMD_HIP(h, hipMemsetAsync(h->d_ke_tile, 0, 2 * 3 * (size_t)h->plan.T * sizeof(double), h->stream));
    }
    if (reproducible(h)) {
        h->rec_stride = kExactWords;
        LJMD_HIP(h, hipMalloc(&h->d_fslab, (size_t)h->plan.nslab_t * kFixedQuantities * h->plan.P * sizeof(__int128)));
        LJMD_HIP(h, hipMalloc(&h->d_fflag, (size_t)h->plan.nslab_t * h->plan.TB * sizeof(unsigned)));
        LJMD_HIP(h, hipMalloc(&h->d_fblk, (size_t)(h->plan.P / kBlock) * kExactWords * sizeof(int64_t)));
        LJMD_HIP(h, hipMalloc(&h->d_frec, kExactWords * sizeof(int64_t)));
    }
    LJMD_HIP(h, hipMalloc(&h->d_ring, (size_t)kRingCap * h->rec_stride * sizeof(double)));
    LJMD_HIP(h, hipMalloc(&h->d_ring_pos, sizeof(unsigned)));
    LJMD_HIP(h, hipMalloc(&h->d_bbox, (size_t)h->plan.T * kBoxStride * sizeof(double)));
    LJMD_HIP(h, hipMalloc(&h->d_mask, (size_t)h->plan.TB * h->plan.W * sizeof(uint64_t)));
    LJMD_HIP(h, hipMalloc(&h->d_idx, (size_t)h->plan.P * sizeof(int)));
    LJMD_HIP(h, hipMalloc(&h->d_idx2, (size_t)h->plan.P * sizeof(int)));
    LJMD_HIP(h, hipMalloc(&h->d_perm, (size_t)h->plan.P * sizeof(int)));
    LJMD_HIP(h, hipMalloc(&h->d_perm2, (size_t)h->plan.P * sizeof(int)));
    LJMD_HIP(h, hipMalloc(&h->d_gid0, (size_t)h->plan.P * sizeof(int)));
    LJMD_HIP(h, launch_iota_offset(h->d_gid0, h->plan.S, h->plan.P, h->rank * h->plan.S, h->stream));
    h->cub_bytes = kd_temp_bytes(h->plan.S);
    LJMD_HIP(h, hipMalloc(&h->d_cub, std::max<size_t>(h->cub_bytes, 16)));
    LJMD_HIP(h, hipMalloc(&h->d_kd_keys, (size_t)h->plan.P * sizeof(unsigned long long)));
    LJMD_HIP(h, hipMalloc(&h->d_kd_keys2, (size_t)h->plan.P * sizeof(unsigned long long)));
    LJMD_HIP(h, hipMalloc(&h->d_kd_offsets, std::max<size_t>(kd.size(), 2) * sizeof(int)));
    if (!kd.empty())
        LJMD_HIP(h, hipMemcpyAsync(h->d_kd_offsets, kd.data(), kd.size() * sizeof(int),
                                   hipMemcpyHostToDevice, h->stream));
    LJMD_HIP(h, hipMemsetAsync(h->d_ring_pos, 0, sizeof(unsigned), h->stream));
    LJMD_HIP(h, hipMemsetAsync(h->d_a, 0, P3, h->stream));
    LJMD_HIP(h, hipMemsetAsync(h->d_ke_part, 0, 3 * (size_t)h->plan.n_ke * sizeof(double), h->stream));
    LJMD_HIP(h, hipHostMalloc(&h->h_stage, P3 * std::max(h->G, 4), hipHostMallocDefault));   // G position blocks, or r, ru, v, a
    LJMD_HIP(h, hipHostMalloc(&h->h_ring, (size_t)kRingCap * h->rec_stride * sizeof(double),
                              hipHostMallocDefault));
    LJMD_HIP(h, hipStreamSynchronize(h->stream));
    return LJMD_OK;
}

void release(ljmd_t *h)
{
    if (!h) return;
    if (h->device >= 0) (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    release_resident(h);
    if (h->comm_stream) (void)hipStreamSynchronize(h->comm_stream);
    if (h->comm) (void)ncclCommDestroy(h->comm);
    if (h->comm_stream) (void)hipStreamDestroy(h->comm_stream);
    if (h->far_stream) {
        (void)hipStreamSynchronize(h->far_stream);
        (void)hipStreamDestroy(h->far_stream);
    }
    if (h->side_stream) {
        (void)hipStreamSynchronize(h->side_stream);
        (void)hipStreamDestroy(h->side_stream);
    }
    if (h->ev_side_go) (void)hipEventDestroy(h->ev_side_go);
    if (h->ev_side_done) (void)hipEventDestroy(h->ev_side_done);
    if (h->ev_far_go) (void)hipEventDestroy(h->ev_far_go);
    if (h->ev_far_done) (void)hipEventDestroy(h->ev_far_done);
    if (h->ev_pos_ready) (void)hipEventDestroy(h->ev_pos_ready);
    if (h->ev_gather_done) (void)hipEventDestroy(h->ev_gather_done);
    for (auto &q : h->ev_pool)
        for (auto &e : q.e) (void)hipEventDestroy(e);
    void *dev[] = {h->d_pos, h->d_ru, h->d_v, h->d_a, h->d_slab, h->d_wg_part, h->d_ke_part, h->d_ring,
                   h->d_ring_pos, h->d_bbox, h->d_mask, h->d_idx, h->d_idx2,
                   h->d_perm, h->d_perm2, h->d_tmp3, h->d_ru2, h->d_v2, h->d_a2, h->d_cub, h->d_slab_j, h->d_flag_j, h->d_fpart, h->d_frecv, h->d_fall,
                   h->d_kd_offsets, h->d_kd_keys, h->d_kd_keys2, h->d_mask_far, h->d_slab_j2, h->d_flag_j2, h->d_fold, h->d_ticket,
                   h->d_desc, h->d_desc_far, h->d_desc2, h->d_red_part, h->d_ke_tile, h->d_pos_tc, h->d_gid0, h->d_mig, h->d_mig_idx, h->d_mig_idx2, h->d_mig_keys,
                   h->d_mig_keys2, h->d_mig_offsets, h->d_mig_cub, h->d_fslab, h->d_fflag, h->d_fblk, h->d_frec};
    for (void *p : dev) (void)hipFree(p);
    if (h->h_stage) (void)hipHostFree(h->h_stage);
    if (h->h_ring) (void)hipHostFree(h->h_ring);
    if (h->copy_stream) {
        (void)hipStreamSynchronize(h->copy_stream);
        (void)hipStreamDestroy(h->copy_stream);
    }
    if (h->ev_snap_ready) (void)hipEventDestroy(h->ev_snap_ready);
    if (h->ev_snap_done) (void)hipEventDestroy(h->ev_snap_done);
    if (h->d_snap) (void)hipFree(h->d_snap);
    if (h->d_snap_perm) (void)hipFree(h->d_snap_perm);
    if (h->h_snap) (void)hipHostFree(h->h_snap);
    if (h->h_snap_perm) (void)hipHostFree(h->h_snap_perm);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

// HBM -> host of any of r, ru, v, a (dsts[3 w + k], NULL = skip) and of the last n_records scalar records, all
// behind ONE stream synchronisation; the arrays are delivered in the caller's original particle order.
int download_state(ljmd_t *h, double *const dsts[12], unsigned n_records)
{
    const size_t P = h->plan.P;
    const double *srcs[4] = {own_block(h), h->d_ru, h->d_v, h->d_a};
    bool want[4];
    for (int w = 0; w < 4; ++w) {
        want[w] = dsts[3 * w] || dsts[3 * w + 1] || dsts[3 * w + 2];
        if (want[w])
            LJMD_HIP(h, hipMemcpyAsync(h->h_stage + (size_t)w * 3 * P, srcs[w], 3 * P * sizeof(double),
                                       hipMemcpyDeviceToHost, h->stream));
    }
    if (h->perm_dirty)
        LJMD_HIP(h, hipMemcpyAsync(h->h_perm.data(), h->d_perm, P * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    if (n_records > 0) {
        const int rc_ = fetch_ring(h, n_records);      // synchronises the stream
        if (rc_ != LJMD_OK) return rc_;
    } else {
        LJMD_HIP(h, hipStreamSynchronize(h->stream));
    }
    h->perm_dirty = false;
    for (int w = 0; w < 4; ++w) {
        if (!want[w]) continue;
        for (int k = 0; k < 3; ++k) {
            double *dst = dsts[3 * w + k];
            if (!dst) continue;
            const double *st = h->h_stage + ((size_t)w * 3 + k) * P;
            for (int i = 0; i < h->plan.P; ++i) {
                const int o = h->h_perm[i];
                if (o < h->plan.S) dst[o] = st[i];           // slot -> original index of the shard
            }
        }
    }
    return LJMD_OK;
}

// stage[ax*P + slot] for the owned shard, slot order = current device order
void stage_permuted(ljmd_t *h, const double *x, const double *y, const double *z, size_t off, double pad)
{
    const double *src[3] = {x + off, y + off, z + off};
    for (int ax = 0; ax < 3; ++ax) {
        double *dst = h->h_stage + (size_t)ax * h->plan.P;
        if (h->migrated) {
            // after an ownership migration the shard is a SET of the caller's particles, not an index range: position o
            // of the engine's order holds particle h_gid0[o] of the arrays given to ljmd_set_state
            const double *glob = src[ax] - off;
            for (int i = 0; i < h->plan.P; ++i) {
                const int o = h->h_perm[i];
                dst[i] = (o < h->plan.S) ? glob[h->h_gid0[o]] : pad;
            }
            continue;
        }
        for (int i = 0; i < h->plan.P; ++i) {
            const int o = h->h_perm[i];
            dst[i] = (o < h->plan.S) ? src[ax][o] : pad;
        }
    }
}

int upload_shard3(ljmd_t *h, double *dst, const double *x, const double *y, const double *z)
{
    int rc_ = refresh_perm(h);
    if (rc_ != LJMD_OK) return rc_;
    stage_permuted(h, x, y, z, (size_t)h->rank * h->plan.S, 0.0);
    LJMD_HIP(h, hipMemcpyAsync(dst, h->h_stage, 3 * (size_t)h->plan.P * sizeof(double), hipMemcpyHostToDevice,
                               h->stream));
    LJMD_HIP(h, hipStreamSynchronize(h->stream));  // staging buffer is reused
    return LJMD_OK;
}

}  // namespace ljmdh
