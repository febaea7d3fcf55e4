"""-m gpu: the van Hove self-correlation accumulated on the device by the batch engine (ljmd_batch_vanhove_*,
BatchEngine.vanhove_*).  Histogram and sums are exact integers: every comparison is equality with tests/vanhove_model.py
(the definition of include/ljmd.h in numpy and Python ints), one model per replica, on the ru get_state returns; the
quotients are R(S) / (n count) bit for bit."""
import numpy as np
import pytest

import tcf_model
import vanhove_model
from ljmd_amd import BatchEngine, Engine, _lib, synthetic
from ljmd_amd._lib import LjmdError
from test_gpu_batch_rdf import MIX, NBINS, SWEEP
from test_gpu_batch_tcf import _code, _flat_state, _replicas, _set, _set_per_replica
from vanhove_model import S2, S4, VanHoveModel

pytestmark = pytest.mark.gpu


def _ru(eng):
    """-> per replica ru [3, n_b] of the resident state; works for both kinds of engine"""
    st = eng.get_state(("ru",))["ru"]
    return [np.stack([st[ax][b] for ax in range(3)]) for b in range(eng.n_replicas)]


def _push(models, eng):
    for m, ru in zip(models, _ru(eng)):
        m.push(ru)


def _take(eng, models):
    eng.vanhove_accumulate()
    _push(models, eng)


def _assert_equals_models(eng, models, ns, flagged=False):
    """vanhove_read_exact == the models' integers, vanhove_read == R(S) / (n count) bitwise, the counts the models', and
    every row of H sums to n count"""
    if flagged:
        with pytest.raises(LjmdError) as ei:
            eng.vanhove_read_exact()
        hist, sums, counts, _ = ei.value.result
        with pytest.raises(LjmdError) as ei:
            eng.vanhove_read()
        hist2, r2, r4, counts2, _ = ei.value.result
    else:
        hist, sums, counts, _ = eng.vanhove_read_exact()
        hist2, r2, r4, counts2, _ = eng.vanhove_read()
    assert np.array_equal(counts, counts2) and np.array_equal(hist, hist2)
    for b, (m, n) in enumerate(zip(models, ns)):
        assert np.array_equal(counts, m.counts), (counts, m.counts)
        assert np.array_equal(hist[b], m.H), b
        assert np.array_equal(hist[b].sum(axis=1), np.uint64(n) * counts.astype(np.uint64)), b
        for kind, got in ((S2, r2), (S4, r4)):
            assert list(sums[b, kind]) == m.S[kind], (b, kind)
            assert got[b].tobytes() == m.result(kind, n).tobytes(), (b, kind, got[b])
    return hist, sums, counts


# ---- 1. accumulation against the model -------------------------------------------------------------------------------
# every kernel class and particles-per-thread mapping (1, 2 and 4), partial waves, the smallest system
@pytest.mark.parametrize("max_lag, stride, nbins", [(8, 1, 128), (5, 3, 7), (7, 2, 1)])
@pytest.mark.parametrize("n, B", [(2, 3), (65, 3), (108, 3), (1025, 3), (2049, 2), (4096, 2)])
def test_accumulation_equals_the_model(n, B, max_lag, stride, nbins):
    p, r, v = _replicas(n, range(300, 300 + B))
    rmax = 0.02 * np.arange(1, B + 1)                  # a few steps move a particle by some 0.01: both branches of the bin
    models = [VanHoveModel(max_lag, stride, nbins, rm) for rm in rmax]
    with BatchEngine(p, B) as eng:
        _set(eng, r, v)
        eng.compute_forces()
        eng.vanhove_configure(max_lag, stride, nbins, rmax)
        _take(eng, models)
        for _ in range(9):
            eng.steps(2, observables=False)
            _take(eng, models)
        hist, sums, counts = _assert_equals_models(eng, models, [n] * B)
        assert eng.vanhove_read()[4] == 10
    assert np.array_equal(counts, tcf_model.reference_counts(10, max_lag, stride))
    assert all(int(sums[b, S2, 0]) == 0 and int(sums[b, S2, max_lag]) > 0 for b in range(B))
    assert not np.array_equal(hist[0], hist[1])         # the replicas differ: each row is its own replica's


# ---- 2. mixed n in one launch group: replicas with fewer threads than the block, one wave idle throughout ------------
def test_mixed_n_in_one_launch_group():
    ns, rhos = (2, 65, 108, 100), (None, 0.6, 0.8, 0.7)
    cfg = [_replicas(2, [81])] + [synthetic.make_config(n, seed=80 + n, rho=rho) for n, rho in zip(ns[1:], rhos[1:])]
    cfg[0] = (cfg[0][0], cfg[0][1][0], cfg[0][2][0])
    rmax = [0.05, 0.01, 0.03, 0.02]
    models = [VanHoveModel(4, 1, 16, rm) for rm in rmax]
    with BatchEngine.per_replica([c[0] for c in cfg]) as eng:
        _set_per_replica(eng, cfg)
        eng.compute_forces()
        eng.vanhove_configure(4, 1, 16, rmax)
        _take(eng, models)
        for _ in range(7):
            eng.steps(3, observables=False)
            _take(eng, models)
        _assert_equals_models(eng, models, ns)


# ---- 3. the LDS maximum, ring revolutions ----------------------------------------------------------------------------
def test_origin_and_bin_caps_and_ring_wrap_around():
    """max_lag = 511 with stride 1 and 1024 bins: 512 ring slots, 511 live origins, the lag-0 entry and 1025 bins -- the
    largest LDS footprint -- and 516 snapshots wrap the ring"""
    n, max_lag = 108, 511
    p, r, v = _replicas(n, [61])
    models = [VanHoveModel(max_lag, 1, 1024, 0.3)]
    with BatchEngine(p, 1) as eng:
        _set(eng, r, v)
        eng.compute_forces()
        eng.vanhove_configure(max_lag, 1, 1024, 0.3)
        for s in range(516):
            if s:
                eng.steps(1, observables=False)
            _take(eng, models)
        _, _, counts = _assert_equals_models(eng, models, [n])
    assert np.array_equal(counts, tcf_model.reference_counts(516, max_lag, 1))


def test_several_ring_revolutions():
    n, B = 108, 2
    p, r, v = _replicas(n, [62, 63])
    models = [VanHoveModel(6, 2, 32, 0.05) for _ in range(B)]
    with BatchEngine(p, B) as eng:
        _set(eng, r, v)
        eng.compute_forces()
        eng.vanhove_configure(6, 2, 32, 0.05)
        for s in range(30):                              # 4 slots: more than three revolutions
            if s:
                eng.steps(1, observables=False)
            _take(eng, models)
        _assert_equals_models(eng, models, [n] * B)


# ---- 4. the overflow column ------------------------------------------------------------------------------------------
def test_overflow_column_takes_a_share():
    n, B = 108, 2
    p, r, v = _replicas(n, [64, 65])
    models = [VanHoveModel(3, 1, 10, 0.02) for _ in range(B)]
    with BatchEngine(p, B) as eng:
        _set(eng, r, v)
        eng.compute_forces()
        eng.vanhove_configure(3, 1, 10, 0.02)
        _take(eng, models)
        for _ in range(4):
            eng.steps(4, observables=False)
            _take(eng, models)
        _assert_equals_models(eng, models, [n] * B)
    for m in models:
        over, all_ = int(m.H[1:, -1].sum()), int(m.H[1:].sum())
        assert 0 < over < all_, (over, all_)              # the inside and the outside branch both ran


# ---- 5. S2 is the MSD of ljmd_batch_tcf_* ----------------------------------------------------------------------------
def test_s2_equals_the_msd_words_on_the_same_handle():
    n, B = 500, 2
    p, r, v = _replicas(n, [66, 67])
    with BatchEngine(p, B) as eng:
        _set(eng, r, v)
        eng.compute_forces()
        eng.vanhove_configure(5, 2, 20, 0.1)
        eng.tcf_configure(5, 2)
        for s in range(9):
            if s:
                eng.steps(2, observables=False)
            eng.vanhove_accumulate()
            eng.tcf_accumulate()
        _, vh, counts, _ = eng.vanhove_read_exact(raw=True)
        tcf, counts2, _ = eng.tcf_read_exact(raw=True)
    assert np.array_equal(counts, counts2) and counts[5] > 0
    assert vh[:, S2].tobytes() == tcf[:, tcf_model.MSD].tobytes() and vh[:, S2, 5].any()


# ---- 6. a replica's integers are its own -----------------------------------------------------------------------------
def _mix_run(cfg, mode=_lib.PRECISION_FP64):
    with BatchEngine.per_replica([c[0] for c in cfg], precision_mode=mode) as eng:
        _set_per_replica(eng, cfg)
        eng.compute_forces()
        eng.vanhove_configure(3, 2, 24, [0.02 + 0.0001 * c[0].n for c in cfg], every=2)
        eng.vanhove_accumulate()
        eng.steps(6, 3)
        eng.vanhove_accumulate()
        hist, words, counts, snaps = eng.vanhove_read_exact(raw=True)
    assert snaps == 5 and np.array_equal(counts, tcf_model.reference_counts(5, 3, 2))
    return hist, words


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_integers_do_not_depend_on_batch_slot_neighbours_streams_or_particle_order(monkeypatch):
    cfg = [synthetic.make_config(n, seed=s, rho=rho) for n, rho, s in MIX]
    B = len(cfg)
    fwd = _mix_run(cfg)
    rev = _mix_run(cfg[::-1])
    for b, c in enumerate(cfg):
        alone = _mix_run([c])
        assert alone[1][0, S2, 2].any()
        assert _same((fwd[0][b], fwd[1][b]), (alone[0][0], alone[1][0])), (b, c[0].n)
        assert _same((rev[0][B - 1 - b], rev[1][B - 1 - b]), (alone[0][0], alone[1][0])), (b, c[0].n)
    # the order of a replica's particles: the reproducible mode's state is a function of the particle set, so the
    # permuted input gives the permuted snapshots -- and integers over the particles do not see the order
    mode = _lib.PRECISION_FP64_REPRODUCIBLE
    small = cfg[:3]
    base = _mix_run(small, mode)
    perm = np.random.Generator(np.random.PCG64(5)).permutation(small[1][0].n)
    shuffled = [small[0], (small[1][0], small[1][1][:, perm], small[1][2][:, perm]), small[2]]
    assert _same(_mix_run(shuffled, mode), base)
    monkeypatch.setenv("LJMD_BATCH_GROUP_STREAMS", "0")
    assert _same(_mix_run(cfg), fwd)


def _fed(mode, ru_series, p, B):
    """the same snapshots, given through set_unwrapped, on a handle of `mode`"""
    with BatchEngine(p, B, precision_mode=mode) as eng:
        _set(eng, *ru_series[0][1:])
        eng.vanhove_configure(4, 1, 16, 0.05)
        for ru, _, _ in ru_series:
            eng.set_unwrapped(ru[:, 0], ru[:, 1], ru[:, 2])
            eng.vanhove_accumulate()
        return eng.vanhove_read_exact(raw=True)[:2]


def test_precision_mode_does_not_matter_and_the_single_engine_agrees():
    n, B = 108, 2
    p, r, v = _replicas(n, [68, 69])
    mode = _lib.PRECISION_FP64_REPRODUCIBLE
    series = []
    with BatchEngine(p, B, precision_mode=mode) as eng:
        _set(eng, r, v)
        eng.compute_forces()
        eng.vanhove_configure(4, 1, 16, 0.05)
        for s in range(7):
            if s:
                eng.steps(3, observables=False)
            eng.vanhove_accumulate()
            series.append((np.stack([np.stack(x) for x in _ru(eng)]), r, v))
        batch = eng.vanhove_read_exact(raw=True)
    # given the same ru, the integers of a handle of either mode
    assert _same(_fed(_lib.PRECISION_FP64, series, p, B), batch[:2])
    assert _same(_fed(mode, series, p, B), batch[:2])
    # the reproducible single engine on the same trajectory (bitwise the batch replica's)
    for b in range(B):
        with Engine(p, precision_mode=mode) as one:
            one.set_state(r[b, 0], r[b, 1], r[b, 2], v[b, 0], v[b, 1], v[b, 2])
            one.compute_forces()
            one.vanhove_configure(4, 1, 16, 0.05)
            for s in range(7):
                if s:
                    one.verlet_steps(3)
                ru = np.stack(one.get_state(("ru",))["ru"])
                assert ru.tobytes() == series[s][0][b].tobytes(), (b, s)          # the precondition
                one.vanhove_accumulate()
            hist, words, counts, snaps = one.vanhove_read_exact(raw=True)
        assert snaps == 7 and np.array_equal(counts, batch[2])
        assert np.array_equal(hist, batch[0][b]) and np.array_equal(words, batch[1][b])


# ---- 7. snapshots taken inside steps() -------------------------------------------------------------------------------
def _sweep_cfg():
    return [synthetic.make_config(n, seed=s, rho=rho) for n, rho, s in SWEEP]


RMAX = [0.04, 0.05, 0.06, 0.07]


@pytest.fixture(scope="module")
def sweep_reference():
    """computed once: the integers of the route accumulate, 4 x { steps(10), accumulate } (checked against the model
    there), and state, scalars, MSD / VACF and g(r) of a handle without the feature"""
    cfg = _sweep_cfg()
    ns = [c[0].n for c in cfg]
    models = [VanHoveModel(6, 1, 40, rm) for rm in RMAX]
    with BatchEngine.per_replica([c[0] for c in cfg]) as eng:
        _set_per_replica(eng, cfg)
        eng.compute_forces()
        eng.vanhove_configure(6, 1, 40, RMAX)
        _take(eng, models)
        for _ in range(4):
            eng.steps(10, observables=False)
            _take(eng, models)
        hist, sums, counts = _assert_equals_models(eng, models, ns)
    with BatchEngine.per_replica([c[0] for c in cfg]) as eng:
        _set_per_replica(eng, cfg)
        eng.compute_forces()
        plain = (eng.steps(40, 20), _flat_state(eng))
    with BatchEngine.per_replica([c[0] for c in cfg]) as eng:
        _set_per_replica(eng, cfg)
        eng.compute_forces()
        eng.rdf_configure(NBINS, every=20)
        eng.tcf_configure(4, 1, every=8)
        eng.steps(40, 20)
        others = (eng.rdf_read(), eng.tcf_read_exact(raw=True), eng.profile_read()["launches"])
    return cfg, (hist, sums, counts), plain, others


@pytest.mark.parametrize("with_others", [False, True])
def test_snapshots_inside_steps(sweep_reference, with_others):
    cfg, (want_hist, want_sums, want_counts), plain, others = sweep_reference
    with BatchEngine.per_replica([c[0] for c in cfg]) as eng:
        _set_per_replica(eng, cfg)
        eng.compute_forces()
        eng.steps(40, 20)
        base_launches = eng.profile_read()["launches"]
    with BatchEngine.per_replica([c[0] for c in cfg]) as eng:
        _set_per_replica(eng, cfg)
        eng.compute_forces()
        eng.vanhove_configure(6, 1, 40, RMAX, every=10)
        if with_others:
            eng.rdf_configure(NBINS, every=20)
            eng.tcf_configure(4, 1, every=8)
        eng.vanhove_accumulate()
        scalars = eng.steps(40, 20)
        prof = eng.profile_read()
        hist, sums, counts, snaps = eng.vanhove_read_exact()
        state = _flat_state(eng)
        if with_others:
            (rdf, n_rdf), tcf, launches = others
            got_rdf, got_n = eng.rdf_read()
            assert got_n == n_rdf == 2 and np.array_equal(got_rdf, rdf)
            got_tcf = eng.tcf_read_exact(raw=True)
            assert got_tcf[2] == tcf[2] == 5 and np.array_equal(got_tcf[0], tcf[0]) and np.array_equal(got_tcf[1], tcf[1])
            # a launch ends at the multiples of 8, 10 and 20: 8 10 16 20 24 30 32 40 -- the same cuts for every group,
            # so beside the launches of the handle without van Hove there are its own four per group
            assert prof["launches"] == launches + 3 * 4 + 3 * 2, (prof, launches)       # + the two extra cuts at 10, 30
        else:
            assert prof["launches"] == base_launches + 3 * 3 + 3 * 4, (prof, base_launches)   # cuts at 10 20 30
        with pytest.raises(LjmdError) as ei:                     # 15 % 10 != 0: refused, nothing launched
            eng.steps(15, 5)
        # the accumulators are asked in their order, van Hove last: beside g(r) with every = 20 that one answers
        asked = "g(r) interval 20" if with_others else "van Hove interval 10 (ljmd_batch_vanhove_configure: every)"
        assert ei.value.code == _lib.LJMD_ERR_INVALID_ARG and f"multiple of the {asked}" in ei.value.message
        assert eng.vanhove_read_exact()[3] == 5
        assert [a.tobytes() for a in _flat_state(eng)] == [a.tobytes() for a in state]
    assert snaps == 5 and np.array_equal(counts, want_counts)
    assert np.array_equal(hist, want_hist) and np.array_equal(sums, want_sums)
    want_scalars, want_state = plain
    for got, ref in zip(scalars, want_scalars):
        assert got.shape == ref.shape and got.tobytes() == ref.tobytes()
    for got, ref in zip(state, want_state):
        assert got.tobytes() == ref.tobytes()


# ---- 8. range --------------------------------------------------------------------------------------------------------
def test_range_flag_names_the_replica_fills_the_arrays_and_reset_clears_it():
    n, B = 108, 3
    p, r, v = _replicas(n, [71, 72, 73])
    models = [VanHoveModel(4, 1, 12, 0.05) for _ in range(B)]
    with BatchEngine(p, B) as eng:
        _set(eng, r, v)
        eng.compute_forces()
        eng.vanhove_configure(4, 1, 12, 0.05)
        _take(eng, models)
        ru = [a.copy() for a in eng.get_state(("ru",))["ru"]]
        ru[0][1, 5] += 1.0e6                                      # r^4 = 1e24 >= 2^40
        eng.set_unwrapped(*ru)
        _take(eng, models)
        assert [m.range_flag for m in models] == [False, True, False]
        with pytest.raises(LjmdError) as ei:
            eng.vanhove_read()
        assert ei.value.code == _lib.LJMD_ERR_RANGE and "replica 1" in ei.value.message, ei.value.message
        hist, _, _ = _assert_equals_models(eng, models, [n] * B, flagged=True)       # filled all the same
        assert hist[1, 1, -1] >= 1 and hist[0, 1].sum() == n
        eng.steps(4, 2)                                           # stepping is not affected, the handle not poisoned
        assert _code(eng.vanhove_read) == _lib.LJMD_ERR_RANGE     # sticky
        eng.vanhove_reset()
        models = [VanHoveModel(4, 1, 12, 0.05) for _ in range(B)]
        _take(eng, models)
        eng.steps(2, observables=False)
        _take(eng, models)
        _assert_equals_models(eng, models, [n] * B)
        assert eng.vanhove_read()[4] == 2


# ---- 9. sequence and guards ------------------------------------------------------------------------------------------
def _refused(eng, args):
    with pytest.raises(LjmdError) as ei:
        eng.vanhove_configure(*args)
    return ei.value.code, ei.value.message


def test_sequence_and_guards():
    n, B = 108, 3
    p, r, v = _replicas(n, [51, 52, 53])
    lib = _lib.load()
    with BatchEngine(p, B) as eng:
        first_msg = "call ljmd_batch_vanhove_configure first"
        assert lib.ljmd_batch_vanhove_accumulate(eng._h) == _lib.LJMD_ERR_STATE       # before configure
        assert first_msg in _lib.batch_last_error(eng._h)
        assert lib.ljmd_batch_vanhove_read(eng._h, None, None, None, None, None) == _lib.LJMD_ERR_STATE
        assert lib.ljmd_batch_vanhove_read_exact(eng._h, None, None, None, None) == _lib.LJMD_ERR_STATE
        assert lib.ljmd_batch_vanhove_reset(eng._h) == _lib.LJMD_ERR_STATE
        eng.vanhove_configure(3, 1, 8, 0.05)
        assert _code(eng.vanhove_accumulate) == _lib.LJMD_ERR_STATE                   # before set_state
        _set(eng, r, v)
        eng.compute_forces()
        # every guard, in its order: an earlier one wins over a later one
        inf, nan = float("inf"), float("nan")
        for args, text in (((-1, 0, 0, 0.0, -1), "max_lag = -1 outside"), ((4097, 0, 0, 0.0, -1), "max_lag = 4097 outside"),
                           ((3, 0, 0, 0.0, -1), "every must be >= 0"), ((3, 0, 0, 0.0, 0), "origin_stride must be >= 1"),
                           ((600, 1, 0, 0.0, 0), "exceeds LJMD_BATCH_VANHOVE_MAX_ORIGINS"),
                           ((3, 1, 0, 0.0, 0), "nbins = 0 outside"), ((3, 1, 1025, 0.0, 0), "nbins = 1025 outside"),
                           ((3, 1, 8, [0.1, 0.0, nan], 0), "replica 1: rmax must be finite and > 0"),
                           ((3, 1, 8, [0.1, 0.2, inf], 0), "replica 2: rmax must be finite and > 0"),
                           ((3, 1, 8, [-1.0, 0.2, 0.1], 0), "replica 0: rmax must be finite and > 0"),
                           ((3, 1, 1024, 1e-310, 0), "replica 0: rmax / nbins is not a normal number")):
            code, msg = _refused(eng, args)
            assert code == _lib.LJMD_ERR_INVALID_ARG and text in msg, (args, msg)
        assert lib.ljmd_batch_vanhove_configure(eng._h, 3, 1, 8, None, 0) == _lib.LJMD_ERR_INVALID_ARG
        assert "rmax is NULL" in _lib.batch_last_error(eng._h)
        hist, sums, counts, snaps = eng.vanhove_read_exact()                          # the refused calls changed nothing
        assert snaps == 0 and hist.shape == (B, 4, 9) and sums.shape == (B, 2, 4)
        assert not counts.any() and not hist.any() and not any(sums.ravel())

        models = [VanHoveModel(3, 1, 8, 0.05) for _ in range(B)]
        _take(eng, models)
        eng.steps(2, observables=False)
        _take(eng, models)
        eng.steps(2, observables=False)
        _take(eng, models)
        first = _assert_equals_models(eng, models, [n] * B)
        hist, sums, counts, snaps = eng.vanhove_read_exact()                          # read clears nothing
        assert snaps == 3 and np.array_equal(hist, first[0]) and np.array_equal(sums, first[1])
        assert lib.ljmd_batch_vanhove_read(eng._h, None, None, None, None, None) == _lib.LJMD_OK   # any pointer may be NULL

        _set(eng, r[::-1].copy(), v[::-1].copy())                                     # a new trajectory: sums kept
        hist, sums, counts, snaps = eng.vanhove_read_exact()
        assert snaps == 3 and np.array_equal(hist, first[0]) and np.array_equal(sums, first[1])
        eng.compute_forces()
        for m in models:
            m.new_trajectory()
        _take(eng, models)                                                            # no origin is live: nothing added
        hist, sums, counts, snaps = eng.vanhove_read_exact()
        assert snaps == 4 and np.array_equal(hist, first[0]) and np.array_equal(counts, first[2])
        eng.steps(2, observables=False)
        _take(eng, models)
        more = _assert_equals_models(eng, models, [n] * B)                            # both trajectories average together
        assert not np.array_equal(more[0], first[0])

        eng.vanhove_configure(5, 2, 4)                                                # reconfigure: new shape, zeroed
        hist, sums, counts, snaps = eng.vanhove_read_exact()
        assert snaps == 0 and hist.shape == (B, 6, 5) and not hist.any() and not counts.any() and not any(sums.ravel())
        eng.vanhove_configure(0)                                                      # off: today's stepping
        eng.steps(10, 5)
        assert lib.ljmd_batch_vanhove_read(eng._h, None, None, None, None, None) == _lib.LJMD_ERR_STATE
        assert _code(eng.vanhove_accumulate) == _lib.LJMD_ERR_STATE
