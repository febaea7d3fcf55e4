// ljmd_records.cpp -- from per-step partial records to the four scalars (epot, ekin, d_epot, dd_epot): the fp64
// combination in fixed rank order, the 192-bit integer combination of the reproducible mode, and the formulas both
// (and the batch engine) end in.
#include "ljmd_engine.h"

namespace ljmdh {

void scalars_from_sums(double s12, double s6, double kx, double ky, double kz, double te, double td, double tdd,
                       double *epot, double *ekin, double *d_epot, double *dd_epot)
{
    if (epot) *epot = 4.0 * (s12 - s6) + te;                          // lj_potential_energy.f90:140,:188,:221
    if (d_epot) *d_epot = 24.0 * (-2.0 * s12 + s6) + td;              // :143,:177,:192,:222
    if (dd_epot) *dd_epot = 24.0 * (26.0 * s12 - 7.0 * s6) + tdd;     // :178,:193,:223
    if (ekin) *ekin = 0.5 * (kx + ky + kz);                           // verlet.f90:93-95
}

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

namespace {
void neg192(uint64_t (&x)[3])
{
    x[0] = ~x[0]; x[1] = ~x[1]; x[2] = ~x[2];
    const uint64_t one[3] = {1, 0, 0};
    add192(x, one);
}

// x k mod 2^192 (k > 0): two's complement wraps consistently, the admissible range never gets near the bound
void scale192(uint64_t (&x)[3], uint64_t k)
{
    unsigned __int128 carry = 0;
    for (int w = 0; w < 3; ++w) {
        const unsigned __int128 p = (unsigned __int128)x[w] * k + carry;
        x[w] = (uint64_t)p;
        carry = p >> 64;
    }
}

// arithmetic shift right by one (the ordered-pair sums are even: u^6_ij and u^6_ji have the same bits)
void half192(uint64_t (&x)[3])
{
    x[0] = (x[0] >> 1) | (x[1] << 63);
    x[1] = (x[1] >> 1) | (x[2] << 63);
    x[2] = (uint64_t)((int64_t)x[2] >> 1);
}
}  // namespace

void scalars_from_exact_sums(const uint64_t (&ordered)[5][3], double te, double td, double tdd, bool have_e, bool have_k,
                             double *epot, double *ekin, double *d_epot, double *dd_epot)
{
    uint64_t sum[5][3];
    std::memcpy(sum, ordered, sizeof sum);
    half192(sum[0]);                             // ordered -> unordered pairs
    half192(sum[1]);
    const double nan = std::numeric_limits<double>::quiet_NaN();
    if (epot) {                                  // 4 R(S12 - S6) + tail_e
        uint64_t x[3] = {sum[1][0], sum[1][1], sum[1][2]};
        neg192(x);
        add192(x, sum[0]);
        *epot = have_e ? 4.0 * fixed_to_double(x) + te : nan;
    }
    if (d_epot) {                                // 24 R(S6 - 2 S12) + tail_d
        uint64_t x[3] = {sum[0][0], sum[0][1], sum[0][2]};
        scale192(x, 2);
        neg192(x);
        add192(x, sum[1]);
        *d_epot = have_e ? 24.0 * fixed_to_double(x) + td : nan;
    }
    if (dd_epot) {                               // 24 R(26 S12 - 7 S6) + tail_dd
        uint64_t x[3] = {sum[0][0], sum[0][1], sum[0][2]}, y[3] = {sum[1][0], sum[1][1], sum[1][2]};
        scale192(x, 26);
        scale192(y, 7);
        neg192(y);
        add192(x, y);
        *dd_epot = have_e ? 24.0 * fixed_to_double(x) + tdd : nan;
    }
    if (ekin) {                                  // 0.5 ((Kx + Ky) + Kz)
        const double kx = fixed_to_double(sum[2]), ky = fixed_to_double(sum[3]), kz = fixed_to_double(sum[4]);
        *ekin = have_k ? 0.5 * ((kx + ky) + kz) : nan;
    }
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
