"""-m gpu: the pressure tensor of every replica recorded on the device by the batch engine (ljmd_batch_stress_*,
BatchEngine.stress_*).  A snapshot of a replica is 12 exact integers: every comparison of words is equality with
tests/stress_model.py (numpy arithmetic, Python ints) on the state get_state returns, or with the single engine's
ljmd_stress_* given the same state."""
import numpy as np
import pytest

import stress_model
from ljmd_amd import BatchEngine, Engine, _lib, synthetic
from ljmd_amd._lib import LjmdError
from reproducible_model import R
from test_gpu_batch_rdf import MIX, NBINS, SWEEP
from test_gpu_batch_tcf import _pair_config, _replicas, _set, _set_per_replica

pytestmark = pytest.mark.gpu

REPRO = _lib.PRECISION_FP64_REPRODUCIBLE


def _rv(eng):
    """-> per replica (r [3, n_b], v [3, n_b]) of the resident state; works for both kinds of engine"""
    st = eng.get_state(("r", "v"))
    return [(np.stack([st["r"][ax][b] for ax in range(3)]), np.stack([st["v"][ax][b] for ax in range(3)]))
            for b in range(eng.n_replicas)]


def _single_engine_words(p, r, v):
    """the 12 integers ljmd_stress_* records for this state on a one-rank engine"""
    with Engine(p) as one:
        one.set_state(r[0], r[1], r[2], v[0], v[1], v[2])
        one.compute_forces()
        one.stress_configure(1)
        one.stress_accumulate()
        return list(one.stress_read_exact()[0])


# ---- 1. one-shot accumulate, homogeneous handles ---------------------------------------------------------------------
# Every kernel class, the 1-, 2- and 4-particles-per-thread mappings, partial waves and the smallest system.
# The two trace identities hold to rounding only.  Their margins were measured on the CPU, on these very configurations,
# between the model's own two sides: tr K = (R(Kxx) + R(Kyy)) + R(Kzz) against a plain numpy sum of v.v, worst 1.8e-16
# relative; 12 tr S against -24 (s6 - 2 s12) from plain numpy sums over the same pairs, worst 1.6e-14 relative to |d_epot|
# (n = 4096, where d_epot is ~1e-2 of its two parts).  A factor 10 over that for the summation order of the device's sums.
TRACE_K_MARGIN = 10 * 1.8e-16
TRACE_S_MARGIN = 10 * 1.6e-14


@pytest.mark.parametrize("n, B", [(2, 3), (65, 3), (108, 3), (500, 3), (1025, 3), (2049, 2), (4096, 2)])
def test_one_shot_words_equal_the_model(n, B):
    p, r, v = _replicas(n, range(300, 300 + B))
    with BatchEngine(p, B) as eng:
        eng.set_tail_corrections(False)
        _set(eng, r, v)
        _e, d_epot, _dd = eng.compute_forces()
        ekin = eng.kinetic_energy()
        eng.stress_configure(1)
        eng.stress_accumulate()
        words = eng.stress_read_exact()
        pd = eng.stress_read()
        raw = eng.stress_read_exact(raw=True)
        state = _rv(eng)
    assert words.shape == (1, B, 12) and pd.shape == (1, B, 6) and raw.shape == (1, B, 12, 3)
    for b, (rb, vb) in enumerate(state):
        assert rb.tobytes() == r[b].tobytes() and vb.tobytes() == v[b].tobytes()
        got = list(words[0, b])
        # where the numpy model would dominate the test's time, one replica against it and the other against ljmd_stress_*
        if n >= 2049 and b > 0:
            want = _single_engine_words(p, rb, vb)
        else:
            want, flag = stress_model.words(rb, vb, p.box_length, p.rc)
            assert not flag
        assert got == want, (b, [c for c in range(12) if got[c] != want[c]])
        assert [stress_model.to_limbs(x) for x in want] == raw[0, b].tolist()
        assert pd[0, b].tobytes() == stress_model.doubles(want, p.box_length).tobytes()
        if n > 2:
            assert all(x != 0 for x in got[3:6] + got[9:12])
        K, S = got[:6], got[6:]
        rel_k = abs(((R(K[0]) + R(K[1])) + R(K[2])) - 2.0 * ekin[b]) / (2.0 * ekin[b])
        rel_s = abs(12.0 * ((R(S[0]) + R(S[1])) + R(S[2])) + d_epot[b]) / abs(d_epot[b])
        print("n = %d, replica %d: |tr K - 2 ekin| / 2 ekin = %.3e, |12 tr S + d_epot| / |d_epot| = %.3e" % (n, b, rel_k, rel_s))
        assert rel_k <= TRACE_K_MARGIN and rel_s <= TRACE_S_MARGIN
    for b in range(1, B):
        assert list(words[0, b]) != list(words[0, 0])           # each row is its own replica's


# ---- 2. the same integers as the single engine -----------------------------------------------------------------------
@pytest.mark.parametrize("mode", [_lib.PRECISION_FP64, REPRO])
@pytest.mark.parametrize("n", [108, 500])
def test_same_integers_as_the_single_engine(n, mode):
    B = 3
    p, r, v = _replicas(n, range(320, 320 + B))
    with BatchEngine(p, B, precision_mode=mode) as eng:
        _set(eng, r, v)
        eng.compute_forces()
        eng.steps(6, observables=False)
        eng.stress_configure(2)
        eng.stress_accumulate()
        words = eng.stress_read_exact()
        state = _rv(eng)
    for b, (rb, vb) in enumerate(state):
        assert list(words[0, b]) == _single_engine_words(p, rb, vb), b


# ---- 3. snapshots taken inside steps(), per-replica handle -----------------------------------------------------------
def _sweep_cfg():
    return [synthetic.make_config(n, seed=s, rho=rho) for n, rho, s in SWEEP]


def _flat_state(eng):
    st = eng.get_state()
    return [np.concatenate(st[key][ax]) for key in ("r", "ru", "v", "a") for ax in range(3)]


def _started(cfg):
    eng = BatchEngine.per_replica([c[0] for c in cfg])
    _set_per_replica(eng, cfg)
    eng.compute_forces()
    return eng


@pytest.fixture(scope="module")
def sweep_reference():
    """computed once: the words of the route 4 x { steps(5), accumulate } (the last snapshot checked against the model),
    state and scalars of a handle without any accumulator, g(r) and MSD / VACF of a handle without the pressure tensor"""
    cfg = _sweep_cfg()
    with _started(cfg) as eng:
        eng.stress_configure(4)
        for _ in range(4):
            eng.steps(5, observables=False)
            eng.stress_accumulate()
        words = eng.stress_read_exact()
        for b, (rb, vb) in enumerate(_rv(eng)):
            want, flag = stress_model.words(rb, vb, cfg[b][0].box_length, cfg[b][0].rc)
            assert not flag and list(words[3, b]) == want, b
    plain = {}
    for every in (10, 4):
        with _started(cfg) as eng:
            plain[every] = (eng.steps(20, every), _flat_state(eng))
    with _started(cfg) as eng:
        eng.rdf_configure(NBINS, every=10)
        eng.tcf_configure(6, 1, every=4)
        eng.steps(20, 10)
        others = (eng.rdf_read(), eng.tcf_read_exact())
    return cfg, words, plain, others


@pytest.mark.parametrize("streams, sample_every, with_others", [("1", 10, False), ("0", 4, False), ("1", 4, True),
                                                                ("0", 10, True)])
def test_snapshots_inside_steps(sweep_reference, monkeypatch, streams, sample_every, with_others):
    cfg, want_words, plain, (want_rdf, want_tcf) = sweep_reference
    monkeypatch.setenv("LJMD_BATCH_GROUP_STREAMS", streams)
    with _started(cfg) as eng:
        eng.stress_configure(6, every=5)
        if with_others:
            eng.rdf_configure(NBINS, every=10)
            eng.tcf_configure(6, 1, every=4)
        scalars = eng.steps(20, sample_every)
        prof = eng.profile_read()
        words = eng.stress_read_exact()
        state = _flat_state(eng)
        if with_others:
            hist, n_hist = eng.rdf_read()
            assert n_hist == want_rdf[1] == 2 and np.array_equal(hist, want_rdf[0])
            sums, counts, snaps = eng.tcf_read_exact()
            assert snaps == want_tcf[2] == 5 and np.array_equal(counts, want_tcf[1]) and np.array_equal(sums, want_tcf[0])
        with pytest.raises(LjmdError) as ei:                     # 12 % 5 != 0: refused, nothing launched
            eng.steps(12, 4)
        assert ei.value.code == _lib.LJMD_ERR_INVALID_ARG and "is not a multiple of the" in ei.value.message
        if not with_others:                                      # (g(r) with every = 10 is asked first)
            assert "pressure tensor interval 5 (ljmd_batch_stress_configure: every)" in ei.value.message
        assert eng.stress_read_exact().shape == (4, len(cfg), 12)
        assert [a.tobytes() for a in _flat_state(eng)] == [a.tobytes() for a in state]
    assert words.shape == want_words.shape == (4, len(cfg), 12) and np.array_equal(words, want_words)
    want_scalars, want_state = plain[sample_every]
    for got, ref in zip(scalars, want_scalars):
        assert got.shape == ref.shape and got.tobytes() == ref.tobytes()
    for got, ref in zip(state, want_state):
        assert got.tobytes() == ref.tobytes()
    # three kernel classes, each with its step launches split at the four snapshots and four pressure tensor launches
    assert prof["launches"] >= 3 * (4 + 4) and prof["kernel_ms"] > 0.0, prof


# ---- 4. a replica's words are its own --------------------------------------------------------------------------------
def _series(eng):
    eng.stress_configure(3, every=2)
    eng.stress_accumulate()
    eng.steps(4, observables=False)
    words = eng.stress_read_exact()
    assert words.shape[0] == 3
    return words


def test_words_do_not_depend_on_batch_size_or_slot():
    n = 108
    p, r, v = _replicas(n, range(340, 340 + 64))
    got = {}
    for B, slot in ((1, 0), (3, 2), (64, 37), (64, 0)):
        rr, vv = r[:B].copy(), v[:B].copy()
        rr[[0, slot]], vv[[0, slot]] = rr[[slot, 0]], vv[[slot, 0]]      # configuration 0 sits in `slot`
        with BatchEngine(p, B) as eng:
            _set(eng, rr, vv)
            eng.compute_forces()
            got[B, slot] = _series(eng)[:, slot]
    first = got[1, 0]
    assert all(int(x) != 0 for x in first.ravel())
    assert list(first[0]) != list(first[1]) != list(first[2])
    for key, w in got.items():
        assert np.array_equal(w, first), key


def test_words_do_not_depend_on_neighbours_or_particle_order():
    cfg = [synthetic.make_config(n, seed=s, rho=rho) for n, rho, s in MIX]

    def run(c, mode=_lib.PRECISION_FP64):
        with BatchEngine.per_replica([x[0] for x in c], precision_mode=mode) as eng:
            _set_per_replica(eng, c)
            eng.compute_forces()
            return _series(eng)

    fwd, rev = run(cfg), run(cfg[::-1])
    for b, c in enumerate(cfg):
        alone = run([c])
        assert np.array_equal(fwd[:, b], alone[:, 0]) and np.array_equal(rev[:, len(cfg) - 1 - b], alone[:, 0]), b
    # the reproducible mode's state is a function of the particle set, so the permuted input gives the permuted
    # snapshots -- and integer sums over particles and pairs do not see the order
    small = cfg[:3]
    base = run(small, REPRO)
    perm = np.random.Generator(np.random.PCG64(5)).permutation(small[1][0].n)
    shuffled = [small[0], (small[1][0], small[1][1][:, perm], small[1][2][:, perm]), small[2]]
    assert np.array_equal(run(shuffled, REPRO), base)


# ---- 5. series bookkeeping -------------------------------------------------------------------------------------------
def _err(call):
    with pytest.raises(LjmdError) as ei:
        call()
    return ei.value.code, ei.value.message


def test_series_bookkeeping():
    n, B = 108, 3
    p, r, v = _replicas(n, [351, 352, 353])
    lib = _lib.load()
    with BatchEngine(p, B) as eng:
        _set(eng, r, v)
        eng.compute_forces()
        eng.stress_configure(3)
        for _ in range(3):
            eng.stress_accumulate()
        code, msg = _err(eng.stress_accumulate)                                     # the fourth
        assert code == _lib.LJMD_ERR_STATE and "full" in msg
        full = eng.stress_read_exact()
        assert full.shape == (3, B, 12) and np.array_equal(full[0], full[1]) and np.array_equal(full[1], full[2])
        assert lib.ljmd_batch_stress_read(eng._h, None, None) == _lib.LJMD_OK       # every pointer may be NULL
        assert lib.ljmd_batch_stress_read_exact(eng._h, None, None) == _lib.LJMD_OK
        eng.stress_reset()
        assert eng.stress_read_exact().shape == (0, B, 12) and eng.stress_read().shape == (0, B, 6)

        eng.stress_configure(3, every=2)                                            # reconfigure: empty, zeroed
        assert eng.stress_read_exact().shape == (0, B, 12)
        before = [a.tobytes() for a in _flat_homogeneous(eng)]
        code, msg = _err(lambda: eng.steps(8, observables=False))                   # 4 snapshots, room for 3
        assert code == _lib.LJMD_ERR_STATE and "full" in msg
        assert [a.tobytes() for a in _flat_homogeneous(eng)] == before              # nothing was launched
        assert eng.stress_read_exact().shape == (0, B, 12)
        eng.steps(6, observables=False)                                             # 3 snapshots fit
        three = eng.stress_read_exact()
        assert three.shape == (3, B, 12) and not np.array_equal(three[0], three[2])
        code, msg = _err(lambda: eng.steps(2, observables=False))
        assert code == _lib.LJMD_ERR_STATE and "full" in msg

        _set(eng, r[::-1].copy(), v[::-1].copy())                                   # the setters keep the series
        eng.set_precision(REPRO)
        eng.set_precision(_lib.PRECISION_FP64)
        _set(eng, r, v)
        eng.set_tail_corrections(False)
        eng.rdf_configure(20)
        eng.tcf_configure(4)
        assert np.array_equal(eng.stress_read_exact(), three)
        eng.stress_reset()
        eng.prepare([5, 6, 7], -500.0, warmup_steps=4)                              # the warm-up takes no snapshot
        assert eng.stress_read_exact().shape == (0, B, 12)
        eng.steps(2, observables=False)                                             # ... and the interval is back
        one = eng.stress_read_exact()
        assert one.shape == (1, B, 12)
        for b, (rb, vb) in enumerate(_rv(eng)):
            want, flag = stress_model.words(rb, vb, p.box_length, p.rc)
            assert not flag and list(one[0, b]) == want, b

        eng.stress_configure(0)                                                     # off
        for call in (lambda: lib.ljmd_batch_stress_accumulate(eng._h), lambda: lib.ljmd_batch_stress_reset(eng._h),
                     lambda: lib.ljmd_batch_stress_read(eng._h, None, None),
                     lambda: lib.ljmd_batch_stress_read_exact(eng._h, None, None)):
            assert call() == _lib.LJMD_ERR_STATE
            assert "ljmd_batch_stress_configure first" in _lib.batch_last_error(eng._h)
        eng.steps(3, observables=False)                                             # today's stepping
        eng.stress_configure(5, every=1)                                            # destroyed while configured
        eng.steps(2, observables=False)


def _flat_homogeneous(eng):
    st = eng.get_state()
    return [np.asarray(a) for key in ("r", "ru", "v", "a") for a in st[key]]


# ---- 6. range --------------------------------------------------------------------------------------------------------
def test_range_flag_names_the_replica_and_reset_clears_it():
    """replica 1's two particles 0.05 sigma apart: f ~ 48 / r^13 is beyond 2^40.  An arithmetic flag: nothing faults"""
    cfg = [_pair_config(s) for s in (361, 362, 363)]
    p = cfg[0][0]
    r, v = np.stack([c[1] for c in cfg]), np.stack([c[2] for c in cfg])
    close = r.copy()
    close[1, :, 1] = close[1, :, 0] + np.array([0.05, 0.0, 0.0])
    assert stress_model.words(close[1], v[1], p.box_length, p.rc)[1]
    with BatchEngine(p, 3) as eng:
        _set(eng, close, v)
        eng.stress_configure(4)
        eng.stress_accumulate()
        for read in (eng.stress_read, eng.stress_read_exact):
            code, msg = _err(read)
            assert code == _lib.LJMD_ERR_RANGE and "replica 1" in msg and "ljmd_batch_stress_reset" in msg, msg
        apart = r.copy()
        apart[1, :, 1] = apart[1, :, 0] + np.array([1.1, 0.0, 0.0])
        _set(eng, apart, v)
        eng.compute_forces()
        assert eng.steps(2, 1)[0].shape == (2, 3)                                   # the handle still steps
        assert _err(eng.stress_read_exact)[0] == _lib.LJMD_ERR_RANGE                # sticky until reset
        eng.stress_reset()
        _set(eng, apart, v)
        eng.stress_accumulate()
        words, pd = eng.stress_read_exact(), eng.stress_read()
    assert words.shape == (1, 3, 12) and pd.shape == (1, 3, 6)
    for b in range(3):
        want, flag = stress_model.words(apart[b], v[b], p.box_length, p.rc)
        assert not flag and list(words[0, b]) == want
        assert pd[0, b].tobytes() == stress_model.doubles(want, p.box_length).tobytes()


# ---- 7. guards in order ----------------------------------------------------------------------------------------------
def test_guards_in_order():
    n, B = 108, 3
    p, r, v = _replicas(n, [371, 372, 373])
    lib = _lib.load()
    assert lib.ljmd_batch_stress_configure(None, -1, -1) == _lib.LJMD_ERR_INVALID_ARG      # the NULL handle comes first
    assert "NULL handle" in _lib.batch_last_error()
    with BatchEngine(p, B, precision_mode=REPRO) as eng:
        for bad in (-1, _lib.BATCH_STRESS_MAX_SNAPSHOTS + 1):
            code, msg = _err(lambda: eng.stress_configure(bad, -1))                  # max_snapshots before every
            assert code == _lib.LJMD_ERR_INVALID_ARG and msg.startswith("ljmd_batch_stress_configure: max_snapshots"), msg
        code, msg = _err(lambda: eng.stress_configure(2, -1))
        assert code == _lib.LJMD_ERR_INVALID_ARG and "every" in msg
        code, msg = _err(eng.stress_accumulate)                                     # before configure
        assert code == _lib.LJMD_ERR_STATE and "ljmd_batch_stress_configure first" in msg
        eng.stress_configure(2)
        code, msg = _err(lambda: eng.stress_configure(-3))                          # a failed guard keeps the configuration
        assert code == _lib.LJMD_ERR_INVALID_ARG and eng.stress_read_exact().shape == (0, B, 12)
        code, msg = _err(eng.stress_accumulate)                                     # before a state
        assert code == _lib.LJMD_ERR_STATE and "no state" in msg
        bad = r.copy()
        bad[1, :, 1] = bad[1, :, 0]
        bad[1, 0, 1] += 0.05                                                        # the reproducible force pass fails ...
        _set(eng, bad, v)
        assert _err(eng.compute_forces)[0] == _lib.LJMD_ERR_RANGE
        code, msg = _err(eng.stress_accumulate)                                     # ... and poisons the handle
        assert code == _lib.LJMD_ERR_STATE and "poisoned" in msg
        assert eng.stress_read_exact().shape == (0, B, 12)                          # a poisoned handle may still be read
        _set(eng, r, v)
        eng.stress_accumulate()
        assert eng.stress_read_exact().shape == (1, B, 12)
