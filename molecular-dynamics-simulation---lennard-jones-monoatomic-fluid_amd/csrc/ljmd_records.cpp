// ljmd_records.cpp -- from an engine's per-step partial records to the four scalars (epot, ekin, d_epot, dd_epot): the
// fp64 combination in fixed rank order and the 192-bit integer combination of the reproducible mode.  The formulas both
// end in are shared with the batch engine: scalars_from_sums / scalars_from_exact_sums, ljmd_common.cpp.
#include "ljmd_engine.h"

namespace ljmdh {

void combine_one(const ljmd_t *h, const double *recs, int n_ranks, double *epot, double *ekin,
                 double *d_epot, double *dd_epot)
{
    double s12 = 0, s6 = 0, kx = 0, ky = 0, kz = 0;
    for (int g = 0; g < n_ranks; ++g) {  // fixed rank order
        const double *r = recs + (size_t)g * kPartialStride;
        s12 += r[0];
        s6 += r[1];
        kx += r[2];
        ky += r[3];
        kz += r[4];
    }
    // (the kernels already normalised s12, s6 to unordered-pair sums: FinalizeArgs::pair_scale)
    // tail corrections: the reference's compile-time switch use_tail_corrections (lj_potential_energy.f90:36,205-219)
    const double te = h->tail_on ? h->tail_e : 0.0, td = h->tail_on ? h->tail_d : 0.0, tdd = h->tail_on ? h->tail_dd : 0.0;
    scalars_from_sums(s12, s6, kx, ky, kz, te, td, tdd, epot, ekin, d_epot, dd_epot);
}

static_assert(LJMD_EXACT_PARTIAL_WORDS == kExactWords, "exact record layout out of sync with include/ljmd.h");

int combine_exact(const ljmd_t *h, const int64_t *recs, int n_ranks, double *epot, double *ekin, double *d_epot,
                  double *dd_epot)
{
    uint64_t sum[5][3] = {};
    int64_t flags = 0;
    for (int g = 0; g < n_ranks; ++g) {          // integers: the rank order does not matter
        const int64_t *r = recs + (size_t)g * kExactWords;
        for (int k = 0; k < 5; ++k) {
            const uint64_t o[3] = {(uint64_t)r[3 * k], (uint64_t)r[3 * k + 1], (uint64_t)r[3 * k + 2]};
            add192(sum[k], o);
        }
        flags |= r[15];
    }
    if (flags & kFlagRange)
        return fail(h, LJMD_ERR_RANGE, "reproducible mode: a pair or velocity term was not finite or |term| >= 2^40 "
                                       "(particles closer than about 0.12 sigma?)");
    const double te = h->tail_on ? h->tail_e : 0.0, td = h->tail_on ? h->tail_d : 0.0, tdd = h->tail_on ? h->tail_dd : 0.0;
    scalars_from_exact_sums(sum, te, td, tdd, !(flags & kFlagNoEnergy), !(flags & kFlagNoKinetic), epot, ekin, d_epot,
                            dd_epot);
    return LJMD_OK;
}

int combine_records(ljmd_t *poison, const ljmd_t *h, const double *recs, int n_ranks, double *epot, double *ekin,
                    double *d_epot, double *dd_epot)
{
    if (!reproducible(h)) {
        combine_one(h, recs, n_ranks, epot, ekin, d_epot, dd_epot);
        return LJMD_OK;
    }
    std::vector<int64_t> w((size_t)n_ranks * kExactWords);
    std::memcpy(w.data(), recs, w.size() * sizeof(int64_t));
    const int rc_ = combine_exact(h, w.data(), n_ranks, epot, ekin, d_epot, dd_epot);
    if (rc_ == LJMD_ERR_RANGE && poison) {
        poison->poisoned = true;
        if (poison != h) poison->err = h->err;
    }
    return rc_;
}

int kinetic_exact(ljmd_t *h, int64_t *rec)
{
    FixedTailArgs ta{};
    ta.P = h->plan.P;
    ta.TB = h->plan.TB;
    ta.v = h->d_v;
    ta.blk = h->d_fblk;
    LJMD_HIP(h, launch_fixed_tail(ta, false, false, true, h->stream));
    FixedFoldArgs fo;
    fo.blk = h->d_fblk;
    fo.n_blk = h->plan.P / kBlock;
    fo.rec = h->d_frec;
    fo.ring_pos = nullptr;
    fo.ring_cap = 1;
    LJMD_HIP(h, launch_fixed_fold(fo, h->stream));
    LJMD_HIP(h, hipMemcpyAsync(rec, h->d_frec, kExactWords * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    LJMD_HIP(h, hipStreamSynchronize(h->stream));
    return LJMD_OK;
}

}  // namespace ljmdh
