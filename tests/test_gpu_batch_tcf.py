"""-m gpu: MSD / VACF accumulated on the device by the batch engine (ljmd_batch_tcf_*, BatchEngine.tcf_*).  The sums are
exact integers: every comparison is equality with tests/tcf_model.py (the definition of include/ljmd.h in numpy and
Python ints) on the snapshots get_state returns, per replica; the quotients are R(S) / (n count) bit for bit."""
import numpy as np
import pytest

import tcf_model
from ljmd_amd import BatchEngine, _lib, md_types, synthetic
from ljmd_amd._lib import LjmdError
from reproducible_model import R
from test_gpu_batch_rdf import MIX, NBINS, SWEEP

pytestmark = pytest.mark.gpu


def _pair_config(seed):
    """n = 2: two particles about 1.1 sigma apart in a box of 4 sigma.  (synthetic.make_config(2) puts them 0.68 sigma
    apart in a box of 1.36: within a few steps the velocities leave the range |term| < 2^40 of the sums.)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    r0 = 1.0 + rng.random(3)
    u = rng.normal(size=3)
    r = np.stack([r0, r0 + (1.05 + 0.1 * rng.random()) * u / np.linalg.norm(u)], axis=1)      # [3, 2]
    v1 = rng.normal(0.0, 0.5, size=3)
    return md_types.init_params(2, 4.0, 0.005, 1.9), r, np.stack([v1, -v1], axis=1)


def _replicas(n, seeds):
    cfg = [_pair_config(s) if n == 2 else synthetic.make_config(n, seed=s) for s in seeds]
    return cfg[0][0], np.stack([c[1] for c in cfg]), np.stack([c[2] for c in cfg])       # p, r[B, 3, n], v[B, 3, n]


def _set(eng, r, v):
    eng.set_state(r[:, 0], r[:, 1], r[:, 2], v[:, 0], v[:, 1], v[:, 2])


def _set_per_replica(eng, cfg):
    eng.set_state(*[[c[1][ax] for c in cfg] for ax in range(3)], *[[c[2][ax] for c in cfg] for ax in range(3)])


def _snapshot(eng):
    """-> per replica (ru [3, n_b], v [3, n_b]) of the resident state; works for both kinds of engine"""
    st = eng.get_state(("ru", "v"))
    return [(np.stack([st["ru"][ax][b] for ax in range(3)]), np.stack([st["v"][ax][b] for ax in range(3)]))
            for b in range(eng.n_replicas)]


def _push(models, eng):
    for m, (ru, v) in zip(models, _snapshot(eng)):
        m.push(ru, v)


def _assert_equals_models(eng, models, ns):
    """tcf_read_exact == the models' integers, tcf_read == R(S) / (n count) bitwise, the counts the models'"""
    sums, counts, _ = eng.tcf_read_exact()
    msd, vacf, counts2, _ = eng.tcf_read()
    assert np.array_equal(counts, counts2)
    for b, (m, n) in enumerate(zip(models, ns)):
        assert not m.range_flag
        assert np.array_equal(counts, m.counts), (counts, m.counts)
        for kind, got in ((tcf_model.MSD, msd), (tcf_model.VACF, vacf)):
            assert list(sums[b, kind]) == m.S[kind], (b, kind)
            want = np.array([R(S) / (n * int(c)) if c else 0.0 for S, c in zip(m.S[kind], counts)])
            assert got[b].tobytes() == want.tobytes(), (b, kind, got[b], want)
    return sums, counts


# ---- 1. accumulation against the model -------------------------------------------------------------------------------
# every kernel class and particles-per-thread mapping (1, 2 and 4), partial waves, the smallest system
@pytest.mark.parametrize("n, B", [(2, 3), (65, 3), (108, 3), (1025, 3), (2049, 2), (4096, 2)])
def test_accumulation_equals_the_model(n, B):
    max_lag, stride = 5, 2
    p, r, v = _replicas(n, range(200, 200 + B))
    models = [tcf_model.TcfModel(max_lag, stride) for _ in range(B)]
    with BatchEngine(p, B) as eng:
        _set(eng, r, v)
        eng.compute_forces()
        eng.tcf_configure(max_lag, stride)
        eng.tcf_accumulate()
        _push(models, eng)
        for _ in range(8):
            eng.steps(2, observables=False)
            eng.tcf_accumulate()
            _push(models, eng)
        sums, counts = _assert_equals_models(eng, models, [n] * B)
        assert eng.tcf_read()[3] == 9
    assert np.array_equal(counts, tcf_model.reference_counts(9, max_lag, stride))
    assert all(int(sums[b, tcf_model.VACF, 0]) > 0 and int(sums[b, tcf_model.MSD, 4]) > 0 for b in range(B))
    assert all(int(sums[b, tcf_model.MSD, 0]) == 0 for b in range(B))
    for kind in (tcf_model.MSD, tcf_model.VACF):
        assert list(sums[0, kind]) != list(sums[1, kind])      # the replicas differ: each row is its own replica's


# ---- 2. snapshots taken inside steps(), per-replica handle -----------------------------------------------------------
def _sweep_cfg():
    return [synthetic.make_config(n, seed=s, rho=rho) for n, rho, s in SWEEP]


def _flat_state(eng):
    st = eng.get_state()
    return [np.concatenate(st[key][ax]) for key in ("r", "ru", "v", "a") for ax in range(3)]


@pytest.fixture(scope="module")
def sweep_reference():
    """computed once: the integers of the route accumulate, 4 x { steps(10), accumulate } (checked against the model
    there), state and scalars of a handle without the feature, and the counts of a handle with g(r) alone"""
    cfg = _sweep_cfg()
    ns = [c[0].n for c in cfg]
    models = [tcf_model.TcfModel(6, 1) for _ in cfg]
    with BatchEngine.per_replica([c[0] for c in cfg]) as eng:
        _set_per_replica(eng, cfg)
        eng.compute_forces()
        eng.tcf_configure(6, 1)
        eng.tcf_accumulate()
        _push(models, eng)
        for _ in range(4):
            eng.steps(10, observables=False)
            eng.tcf_accumulate()
            _push(models, eng)
        sums, counts = _assert_equals_models(eng, models, ns)
    with BatchEngine.per_replica([c[0] for c in cfg]) as eng:
        _set_per_replica(eng, cfg)
        eng.compute_forces()
        plain = (eng.steps(40, 20), _flat_state(eng))
    with BatchEngine.per_replica([c[0] for c in cfg]) as eng:
        _set_per_replica(eng, cfg)
        eng.compute_forces()
        eng.rdf_configure(NBINS, every=20)
        eng.steps(40, 20)
        hist = eng.rdf_read()
    return cfg, sums, counts, plain, hist


@pytest.mark.parametrize("with_rdf", [False, True])
def test_snapshots_inside_steps(sweep_reference, with_rdf):
    cfg, want_sums, want_counts, plain, want_hist = sweep_reference
    with BatchEngine.per_replica([c[0] for c in cfg]) as eng:
        _set_per_replica(eng, cfg)
        eng.compute_forces()
        eng.tcf_configure(6, 1, every=10)
        if with_rdf:
            eng.rdf_configure(NBINS, every=20)
        eng.tcf_accumulate()
        scalars = eng.steps(40, 20)
        prof = eng.profile_read()
        sums, counts, snaps = eng.tcf_read_exact()
        state = _flat_state(eng)
        if with_rdf:
            hist, n_hist = eng.rdf_read()
            assert n_hist == want_hist[1] == 2 and np.array_equal(hist, want_hist[0])
        with pytest.raises(LjmdError) as ei:                     # 15 % 10 != 0: refused, nothing launched
            eng.steps(15, 5)
        assert ei.value.code == _lib.LJMD_ERR_INVALID_ARG and "multiple" in ei.value.message
        assert eng.tcf_read_exact()[2] == 5
        assert [a.tobytes() for a in _flat_state(eng)] == [a.tobytes() for a in state]
    assert snaps == 5 and np.array_equal(counts, want_counts)
    assert np.array_equal(sums, want_sums)
    want_scalars, want_state = plain
    for got, ref in zip(scalars, want_scalars):
        assert got.shape == ref.shape and got.tobytes() == ref.tobytes()
    for got, ref in zip(state, want_state):
        assert got.tobytes() == ref.tobytes()
    # three kernel classes, each with its four MSD / VACF launches (and two g(r) launches)
    assert prof["launches"] >= 3 * (4 + 4 + (2 if with_rdf else 0)), prof


# ---- 3. a replica's sums are its own ---------------------------------------------------------------------------------
def _mix_sums(cfg, mode=_lib.PRECISION_FP64):
    with BatchEngine.per_replica([c[0] for c in cfg], precision_mode=mode) as eng:
        _set_per_replica(eng, cfg)
        eng.compute_forces()
        eng.tcf_configure(3, 2, every=2)
        eng.tcf_accumulate()
        eng.steps(6, 3)
        eng.tcf_accumulate()
        sums, counts, snaps = eng.tcf_read_exact()
    assert snaps == 5 and np.array_equal(counts, tcf_model.reference_counts(5, 3, 2))
    return sums


def test_sums_do_not_depend_on_batch_slot_neighbours_streams_or_particle_order(monkeypatch):
    cfg = [synthetic.make_config(n, seed=s, rho=rho) for n, rho, s in MIX]
    B = len(cfg)
    fwd = _mix_sums(cfg)
    rev = _mix_sums(cfg[::-1])
    for b, c in enumerate(cfg):
        alone = _mix_sums([c])
        assert int(alone[0, tcf_model.MSD, 2]) > 0
        assert np.array_equal(fwd[b], alone[0]), (b, c[0].n)
        assert np.array_equal(rev[B - 1 - b], alone[0]), (b, c[0].n)
    # the order of a replica's particles: the reproducible mode's state is a function of the particle set, so the
    # permuted input gives the permuted snapshots -- and integer sums over the particles do not see the order
    mode = _lib.PRECISION_FP64_REPRODUCIBLE
    small = cfg[:3]
    base = _mix_sums(small, mode)
    perm = np.random.Generator(np.random.PCG64(5)).permutation(small[1][0].n)
    shuffled = [small[0], (small[1][0], small[1][1][:, perm], small[1][2][:, perm]), small[2]]
    assert np.array_equal(_mix_sums(shuffled, mode), base)
    monkeypatch.setenv("LJMD_BATCH_GROUP_STREAMS", "0")
    assert np.array_equal(_mix_sums(cfg), fwd)


# ---- 4. reproducible handles -----------------------------------------------------------------------------------------
def test_reproducible_handle():
    n, B, max_lag, stride = 108, 3, 3, 1
    mode = _lib.PRECISION_FP64_REPRODUCIBLE
    p, r, v = _replicas(n, [41, 42, 43])
    models = [tcf_model.TcfModel(max_lag, stride) for _ in range(B)]
    with BatchEngine(p, B, precision_mode=mode) as eng:
        _set(eng, r, v)
        eng.compute_forces()
        eng.tcf_configure(max_lag, stride, every=4)
        eng.tcf_accumulate()
        _push(models, eng)
        for _ in range(3):
            eng.steps(4, 2)
            _push(models, eng)
        eng.steps(8, 8)                                           # two snapshots in one call: the model gets the last
        sums, counts, snaps = eng.tcf_read_exact()
        state = [np.asarray(a) for key in ("r", "ru", "v", "a") for a in eng.get_state()[key]]
    assert snaps == 6
    with BatchEngine(p, B, precision_mode=mode) as eng:           # the same trajectory without the feature
        _set(eng, r, v)
        eng.compute_forces()
        eng.steps(16, observables=False)
        mid = _snapshot(eng)
        eng.steps(4, observables=False)
        last = _snapshot(eng)
        want_state = [np.asarray(a) for key in ("r", "ru", "v", "a") for a in eng.get_state()[key]]
    for got, ref in zip(state, want_state):
        assert got.tobytes() == ref.tobytes()
    for b, m in enumerate(models):
        m.push(*mid[b])
        m.push(*last[b])
        assert np.array_equal(counts, m.counts)
        for kind in (tcf_model.MSD, tcf_model.VACF):
            assert list(sums[b, kind]) == m.S[kind], (b, kind)


# ---- 5. the origin cap -----------------------------------------------------------------------------------------------
def test_origin_cap_and_ring_wrap_around():
    """max_lag = 511 with stride 1: 512 ring slots, 511 live origins and the lag-0 entry -- the largest LDS footprint --
    and 520 snapshots wrap the ring"""
    n, B, max_lag = 64, 2, 511
    p, r, v = _replicas(n, [61, 62])
    models = [tcf_model.TcfModel(max_lag, 1) for _ in range(B)]
    with BatchEngine(p, B) as eng:
        _set(eng, r, v)
        eng.compute_forces()
        for bad in ((512, 1), (4097, 16), (1024, 2)):
            with pytest.raises(LjmdError) as ei:
                eng.tcf_configure(*bad)
            assert ei.value.code == _lib.LJMD_ERR_INVALID_ARG
        eng.tcf_configure(max_lag, 1)
        for s in range(520):
            if s:
                eng.steps(1, observables=False)
            eng.tcf_accumulate()
            _push(models, eng)
        _, counts = _assert_equals_models(eng, models, [n] * B)
    assert np.array_equal(counts, tcf_model.reference_counts(520, max_lag, 1))


# ---- 6. range --------------------------------------------------------------------------------------------------------
def test_range_flag_names_the_replica_and_reset_clears_it():
    n, B = 108, 3
    p, r, v = _replicas(n, [71, 72, 73])
    with BatchEngine(p, B) as eng:
        _set(eng, r, v)
        eng.compute_forces()
        eng.tcf_configure(4, 1)
        eng.tcf_accumulate()
        ru = [a.copy() for a in eng.get_state(("ru",))["ru"]]
        ru[0][1, 5] += 2.0 ** 21                                  # d^2 = 2^42 >= 2^40
        eng.set_unwrapped(*ru)
        eng.tcf_accumulate()
        for read in (eng.tcf_read, eng.tcf_read_exact):
            with pytest.raises(LjmdError) as ei:
                read()
            assert ei.value.code == _lib.LJMD_ERR_RANGE and "replica 1" in ei.value.message, ei.value.message
        eng.steps(4, 2)                                           # stepping is not affected, the handle not poisoned
        with pytest.raises(LjmdError) as ei:                      # sticky
            eng.tcf_read()
        assert ei.value.code == _lib.LJMD_ERR_RANGE
        eng.tcf_reset()
        models = [tcf_model.TcfModel(4, 1) for _ in range(B)]
        eng.tcf_accumulate()
        _push(models, eng)
        eng.steps(2, observables=False)
        eng.tcf_accumulate()
        _push(models, eng)
        _assert_equals_models(eng, models, [n] * B)
        assert eng.tcf_read()[3] == 2


# ---- 7. sequence and guards ------------------------------------------------------------------------------------------
def _code(call):
    with pytest.raises(LjmdError) as ei:
        call()
    return ei.value.code


def test_sequence_and_guards():
    n, B = 108, 3
    p, r, v = _replicas(n, [51, 52, 53])
    lib = _lib.load()
    with BatchEngine(p, B) as eng:
        assert lib.ljmd_batch_tcf_accumulate(eng._h) == _lib.LJMD_ERR_STATE          # before configure
        assert lib.ljmd_batch_tcf_read(eng._h, None, None, None, None) == _lib.LJMD_ERR_STATE
        assert lib.ljmd_batch_tcf_read_exact(eng._h, None, None, None) == _lib.LJMD_ERR_STATE
        assert lib.ljmd_batch_tcf_reset(eng._h) == _lib.LJMD_ERR_STATE
        eng.tcf_configure(3, 1)
        assert _code(eng.tcf_accumulate) == _lib.LJMD_ERR_STATE                      # before set_state
        _set(eng, r, v)
        eng.compute_forces()
        for bad in ((-1, 1, 0), (4097, 16, 0), (3, 0, 0), (3, 1, -1), (600, 1, 0)):
            assert _code(lambda: eng.tcf_configure(*bad)) == _lib.LJMD_ERR_INVALID_ARG
        sums, counts, snaps = eng.tcf_read_exact()                                   # the refused calls changed nothing
        assert snaps == 0 and sums.shape == (B, 2, 4) and not counts.any() and not any(sums.ravel())

        models = [tcf_model.TcfModel(3, 1) for _ in range(B)]

        def take():
            eng.tcf_accumulate()
            _push(models, eng)

        take()
        eng.steps(2, observables=False)
        take()
        eng.steps(2, observables=False)
        take()
        first, counts = _assert_equals_models(eng, models, [n] * B)
        again, counts2, snaps = eng.tcf_read_exact()                                 # read clears nothing
        assert snaps == 3 and np.array_equal(again, first) and np.array_equal(counts2, counts)
        assert lib.ljmd_batch_tcf_read(eng._h, None, None, None, None) == _lib.LJMD_OK   # every pointer may be NULL

        _set(eng, r[::-1].copy(), v[::-1].copy())                                    # a new trajectory: sums kept
        kept, counts2, snaps = eng.tcf_read_exact()
        assert snaps == 3 and np.array_equal(kept, first) and np.array_equal(counts2, counts)
        eng.compute_forces()
        for m in models:
            m.new_trajectory()
        take()                                                                       # no origin is live: nothing added
        same, counts2, snaps = eng.tcf_read_exact()
        assert snaps == 4 and np.array_equal(same, first) and np.array_equal(counts2, counts)
        eng.steps(2, observables=False)
        take()
        more, _ = _assert_equals_models(eng, models, [n] * B)                        # both trajectories average together
        assert not np.array_equal(more, first)

        eng.tcf_configure(5, 2)                                                      # reconfigure: new shape, zeroed
        sums, counts, snaps = eng.tcf_read_exact()
        assert snaps == 0 and sums.shape == (B, 2, 6) and not counts.any() and not any(sums.ravel())
        eng.tcf_configure(0)                                                         # off: today's stepping
        eng.steps(10, 5)
        assert lib.ljmd_batch_tcf_read(eng._h, None, None, None, None) == _lib.LJMD_ERR_STATE
        assert _code(eng.tcf_accumulate) == _lib.LJMD_ERR_STATE
