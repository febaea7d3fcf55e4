"""-m gpu: the heat flux of every replica recorded on the device by the batch engine (ljmd_batch_heatflux_*,
BatchEngine.heatflux_*).  A snapshot of a replica is 9 exact integers: every comparison of words is equality with
tests/heatflux_model.py (numpy arithmetic, Python ints) on the state get_state returns, or with the single engine's
ljmd_heatflux_* given the same state."""
import numpy as np
import pytest

import heatflux_model
from ljmd_amd import BatchEngine, Engine, _lib, synthetic
from ljmd_amd._lib import LjmdError
from test_gpu_batch_rdf import MIX, NBINS, SWEEP
from test_gpu_batch_tcf import _replicas, _set, _set_per_replica

pytestmark = pytest.mark.gpu

REPRO = _lib.PRECISION_FP64_REPRODUCIBLE


def _rv(eng):
    """-> per replica (r [3, n_b], v [3, n_b]) of the resident state; works for both kinds of engine"""
    st = eng.get_state(("r", "v"))
    return [(np.stack([st["r"][ax][b] for ax in range(3)]), np.stack([st["v"][ax][b] for ax in range(3)]))
            for b in range(eng.n_replicas)]


def _model(p, rb, vb):
    want, flag = heatflux_model.words(rb, vb, p.box_length, p.rc)
    assert not flag
    return want


def _single_engine_words(p, r, v, mode=_lib.PRECISION_FP64):
    """the 9 integers ljmd_heatflux_* records for this state on a one-rank engine"""
    with Engine(p, precision_mode=mode) as one:
        one.set_state(r[0], r[1], r[2], v[0], v[1], v[2])
        one.compute_forces()
        one.heatflux_configure(1)
        one.heatflux_accumulate()
        return list(one.heatflux_read_exact()[0])


# ---- 1. one-shot accumulate, homogeneous handles ---------------------------------------------------------------------
# The first size of every kernel class, the 1-, 2- and 4-particles-per-thread mappings, a partial wave and the smallest
# system.  n = 2049 and 4096 have their columns in two LDS chunks: every pair across the chunk boundary counts once.
@pytest.mark.parametrize("n, B", [(2, 3), (65, 3), (108, 3), (500, 3), (1025, 3), (2049, 2), (4096, 2)])
def test_one_shot_words_equal_the_model(n, B):
    p, r, v = _replicas(n, range(400, 400 + B))
    if n == 2:      # the pair's velocities are opposite, w = 0 and every sum 0: a drift of its own for every replica
        v = v + np.array([[0.3, -0.2, 0.1], [-0.4, 0.1, 0.25], [0.15, 0.35, -0.3]])[:, :, None]
    with BatchEngine(p, B) as eng:
        _set(eng, r, v)
        eng.heatflux_configure(1)
        eng.heatflux_accumulate()
        words = eng.heatflux_read_exact()
        j, parts = eng.heatflux_read()
        raw = eng.heatflux_read_exact(raw=True)
        state = _rv(eng)
    assert words.shape == (1, B, 9) and j.shape == (1, B, 3) and parts.shape == (1, B, 3, 3) and raw.shape == (1, B, 9, 3)
    for b, (rb, vb) in enumerate(state):
        assert rb.tobytes() == r[b].tobytes() and vb.tobytes() == v[b].tobytes()
        got = list(words[0, b])
        want = _model(p, rb, vb)
        assert got == want, (b, [heatflux_model.ROWS[c] for c in range(9) if got[c] != want[c]])
        assert [heatflux_model.to_limbs(x) for x in want] == raw[0, b].tolist()
        want_j, want_parts = heatflux_model.doubles(want, p.box_length)
        assert j[0, b].tobytes() == want_j.tobytes() and parts[0, b].tobytes() == want_parts.tobytes()
        assert all(x != 0 for x in got)
    for b in range(1, B):
        assert list(words[0, b]) != list(words[0, 0])           # each row is its own replica's


# ---- 2. the same integers as the single engine -----------------------------------------------------------------------
@pytest.mark.parametrize("mode", [_lib.PRECISION_FP64, REPRO])
@pytest.mark.parametrize("n", [108, 500])
def test_same_integers_as_the_single_engine(n, mode):
    B = 3
    p, r, v = _replicas(n, range(420, 420 + B))
    with BatchEngine(p, B, precision_mode=mode) as eng:
        _set(eng, r, v)
        eng.compute_forces()
        eng.steps(6, observables=False)
        eng.heatflux_configure(2)
        eng.heatflux_accumulate()
        words = eng.heatflux_read_exact()
        state = _rv(eng)
    for b, (rb, vb) in enumerate(state):
        assert list(words[0, b]) == _single_engine_words(p, rb, vb, mode), b


# ---- 3. snapshots taken inside steps(), per-replica handle of three kernel classes -----------------------------------
STEPS, SAMPLE = 20, 5


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


def _configure_others(eng):
    eng.rdf_configure(NBINS, every=5)
    eng.tcf_configure(6, 1, every=2)
    eng.stress_configure(4, every=20)


def _read_others(eng):
    return eng.rdf_read(), eng.tcf_read_exact(), eng.stress_read_exact()


@pytest.fixture(scope="module")
def sweep_reference():
    """computed once, on handles without the heat flux: the model's words on the state a plain run has after every 2nd
    step (those after steps 4, 8, .. and 10, 20 are used), scalars and final state of a plain run, and the other three
    observables of a run that has them alone"""
    cfg = _sweep_cfg()
    assert len({_batch_class(c[0].n) for c in cfg}) >= 2
    model = {}
    with _started(cfg) as eng:
        for step in range(2, STEPS + 1, 2):
            eng.steps(2, observables=False)
            if step % 4 == 0 or step % 10 == 0:
                model[step] = [_model(cfg[b][0], rb, vb) for b, (rb, vb) in enumerate(_rv(eng))]
        stepped = _flat_state(eng)
    with _started(cfg) as eng:
        plain = (eng.steps(STEPS, SAMPLE), _flat_state(eng))
    assert [a.tobytes() for a in stepped] == [a.tobytes() for a in plain[1]]     # the segments are the run
    with _started(cfg) as eng:
        _configure_others(eng)
        eng.steps(STEPS, SAMPLE)
        others = _read_others(eng)
    return cfg, model, plain, others


def _batch_class(n):
    """the kernel class of a replica of n particles (csrc/ljmd_batch.h: batch_class)"""
    return 0 if n <= 128 else 1 if n <= 512 else 2 if n <= 1024 else 3 if n <= 2048 else 4


def _same(a, b):
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return np.array_equal(a, b)


@pytest.mark.parametrize("streams, every, with_others", [("1", 10, False), ("0", 4, False), ("1", 4, True),
                                                         ("0", 10, True)])
def test_snapshots_inside_steps(sweep_reference, monkeypatch, streams, every, with_others):
    cfg, model, (want_scalars, want_state), want_others = sweep_reference
    monkeypatch.setenv("LJMD_BATCH_GROUP_STREAMS", streams)
    rows = STEPS // every
    with _started(cfg) as eng:
        eng.heatflux_configure(rows + 1, every=every)
        if with_others:
            _configure_others(eng)
        scalars = eng.steps(STEPS, SAMPLE)
        prof = eng.profile_read()
        words = eng.heatflux_read_exact()
        state = _flat_state(eng)
        if with_others:
            assert _same(_read_others(eng), want_others)
        else:
            with pytest.raises(LjmdError) as ei:                 # not a multiple of every: refused, nothing launched
                eng.steps(every + 1, observables=False)
            assert ei.value.code == _lib.LJMD_ERR_INVALID_ARG
            assert "heat flux interval %d (ljmd_batch_heatflux_configure: every)" % every in ei.value.message
            assert eng.heatflux_read_exact().shape == (rows, len(cfg), 9)
            assert [a.tobytes() for a in _flat_state(eng)] == [a.tobytes() for a in state]
    assert words.shape == (rows, len(cfg), 9)
    for k in range(rows):
        for b in range(len(cfg)):
            assert list(words[k, b]) == model[(k + 1) * every][b], (k, b)
    for got, ref in zip(scalars, want_scalars):
        assert got.shape == ref.shape and got.tobytes() == ref.tobytes()
    for got, ref in zip(state, want_state):
        assert got.tobytes() == ref.tobytes()
    # three kernel classes, each with its step launches split at the snapshots and one heat flux launch per snapshot
    assert prof["launches"] >= 3 * 2 * rows and prof["kernel_ms"] > 0.0, prof


# ---- 4. a replica's words are its own --------------------------------------------------------------------------------
def _series(eng):
    eng.heatflux_configure(3, every=2)
    eng.heatflux_accumulate()
    eng.steps(4, observables=False)
    words = eng.heatflux_read_exact()
    assert words.shape[0] == 3
    return words


def test_words_do_not_depend_on_batch_size_or_slot():
    n = 108
    p, r, v = _replicas(n, range(440, 440 + 64))
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


def _flat_homogeneous(eng):
    st = eng.get_state()
    return [np.asarray(a) for key in ("r", "ru", "v", "a") for a in st[key]]


def test_series_bookkeeping():
    n, B = 108, 3
    p, r, v = _replicas(n, [451, 452, 453])
    lib = _lib.load()
    with BatchEngine(p, B) as eng:
        _set(eng, r, v)
        eng.compute_forces()
        eng.heatflux_configure(3)
        for _ in range(3):
            eng.heatflux_accumulate()
        code, msg = _err(eng.heatflux_accumulate)                                   # the fourth
        assert code == _lib.LJMD_ERR_STATE and "full" in msg
        full = eng.heatflux_read_exact()
        assert full.shape == (3, B, 9) and np.array_equal(full[0], full[1]) and np.array_equal(full[1], full[2])
        assert lib.ljmd_batch_heatflux_read(eng._h, None, None, None) == _lib.LJMD_OK   # every pointer may be NULL
        assert lib.ljmd_batch_heatflux_read_exact(eng._h, None, None) == _lib.LJMD_OK
        jj = np.empty((3, B, 3))                                                     # j without parts
        assert lib.ljmd_batch_heatflux_read(eng._h, jj.ctypes.data_as(_lib.c_double_p), None, None) == _lib.LJMD_OK
        assert jj.tobytes() == eng.heatflux_read()[0].tobytes()
        eng.heatflux_reset()
        assert eng.heatflux_read_exact().shape == (0, B, 9)
        j0, parts0 = eng.heatflux_read()
        assert j0.shape == (0, B, 3) and parts0.shape == (0, B, 3, 3)

        eng.heatflux_configure(3, every=2)                                          # reconfigure: empty, zeroed
        assert eng.heatflux_read_exact().shape == (0, B, 9)
        before = [a.tobytes() for a in _flat_homogeneous(eng)]
        code, msg = _err(lambda: eng.steps(8, observables=False))                   # 4 snapshots, room for 3
        assert code == _lib.LJMD_ERR_STATE and "full" in msg
        assert [a.tobytes() for a in _flat_homogeneous(eng)] == before              # nothing was launched
        assert eng.heatflux_read_exact().shape == (0, B, 9)
        eng.steps(6, observables=False)                                             # 3 snapshots fit
        three = eng.heatflux_read_exact()
        assert three.shape == (3, B, 9) and not np.array_equal(three[0], three[2])
        code, msg = _err(lambda: eng.steps(2, observables=False))
        assert code == _lib.LJMD_ERR_STATE and "full" in msg

        _set(eng, r[::-1].copy(), v[::-1].copy())                                   # the setters keep the series
        eng.set_precision(REPRO)
        eng.set_precision(_lib.PRECISION_FP64)
        _set(eng, r, v)
        eng.set_tail_corrections(False)
        eng.rdf_configure(20)
        eng.tcf_configure(4)
        eng.stress_configure(2)
        assert np.array_equal(eng.heatflux_read_exact(), three)
        eng.heatflux_reset()
        eng.prepare([5, 6, 7], -500.0, warmup_steps=4)                              # the warm-up takes no snapshot
        assert eng.heatflux_read_exact().shape == (0, B, 9)
        eng.steps(2, observables=False)                                             # ... and the interval is back
        one = eng.heatflux_read_exact()
        assert one.shape == (1, B, 9)
        for b, (rb, vb) in enumerate(_rv(eng)):
            assert list(one[0, b]) == _model(p, rb, vb), b

        eng.heatflux_configure(0)                                                   # off
        for call in (lambda: lib.ljmd_batch_heatflux_accumulate(eng._h), lambda: lib.ljmd_batch_heatflux_reset(eng._h),
                     lambda: lib.ljmd_batch_heatflux_read(eng._h, None, None, None),
                     lambda: lib.ljmd_batch_heatflux_read_exact(eng._h, None, None)):
            assert call() == _lib.LJMD_ERR_STATE
            assert "ljmd_batch_heatflux_configure first" in _lib.batch_last_error(eng._h)
        eng.steps(3, observables=False)                                             # today's stepping
        eng.heatflux_configure(5, every=1)                                          # destroyed while configured
        eng.steps(2, observables=False)


# ---- 6. range --------------------------------------------------------------------------------------------------------
def test_range_flag_names_the_replica_and_reset_clears_it():
    """replica 1 has one velocity component of 2^41: its k2 and w are beyond 2^40.  An arithmetic flag: nothing faults"""
    n, B = 108, 3
    p, r, v = _replicas(n, [461, 462, 463])
    fast = v.copy()
    fast[1, 0, 5] = 2.0 ** 41
    want = [heatflux_model.words(r[b], fast[b], p.box_length, p.rc) for b in range(B)]
    assert [flag for _w, flag in want] == [False, True, False]
    lib = _lib.load()
    with BatchEngine(p, B) as eng, BatchEngine(p, B) as plain:
        for e in (eng, plain):
            _set(e, r, fast)
            e.compute_forces()
        eng.heatflux_configure(4, every=1)
        eng.heatflux_accumulate()
        for read in (eng.heatflux_read, eng.heatflux_read_exact):
            code, msg = _err(read)
            assert code == _lib.LJMD_ERR_RANGE and "replica 1" in msg and "ljmd_batch_heatflux_reset" in msg, msg
        # read_exact has delivered the words all the same: the other replicas' rows are the model's, and so is the flagged
        # one's, whose out-of-range terms entered as 0
        raw = np.zeros((4, B, 9, 3), dtype=np.int64)
        assert lib.ljmd_batch_heatflux_read_exact(eng._h, raw.ctypes.data_as(_lib.c_int64_p), None) == _lib.LJMD_ERR_RANGE
        for b in range(B):
            assert raw[0, b].tolist() == [heatflux_model.to_limbs(x) for x in want[b][0]], b
        got, ref = eng.steps(2, 1), plain.steps(2, 1)                               # stepping is unaffected
        assert all(a.tobytes() == c.tobytes() for a, c in zip(got, ref))
        assert [a.tobytes() for a in _flat_homogeneous(eng)] == [a.tobytes() for a in _flat_homogeneous(plain)]
        assert _err(eng.heatflux_read_exact)[0] == _lib.LJMD_ERR_RANGE              # sticky until reset
        eng.heatflux_reset()
        _set(eng, r, v)
        eng.heatflux_accumulate()
        words = eng.heatflux_read_exact()
        j, parts = eng.heatflux_read()
    assert words.shape == (1, B, 9) and j.shape == (1, B, 3)
    for b in range(B):
        w = _model(p, r[b], v[b])
        assert list(words[0, b]) == w
        want_j, want_parts = heatflux_model.doubles(w, p.box_length)
        assert j[0, b].tobytes() == want_j.tobytes() and parts[0, b].tobytes() == want_parts.tobytes()


# ---- 7. guards in order ----------------------------------------------------------------------------------------------
def test_guards_in_order():
    n, B = 108, 3
    p, r, v = _replicas(n, [471, 472, 473])
    lib = _lib.load()
    assert lib.ljmd_batch_heatflux_configure(None, -1, -1) == _lib.LJMD_ERR_INVALID_ARG    # the NULL handle comes first
    assert "NULL handle" in _lib.batch_last_error()
    with BatchEngine(p, B, precision_mode=REPRO) as eng:
        for bad in (-1, _lib.BATCH_HEATFLUX_MAX_SNAPSHOTS + 1):
            code, msg = _err(lambda: eng.heatflux_configure(bad, -1))                # max_snapshots before every
            assert code == _lib.LJMD_ERR_INVALID_ARG and msg.startswith("ljmd_batch_heatflux_configure: max_snapshots"), msg
        code, msg = _err(lambda: eng.heatflux_configure(2, -1))
        assert code == _lib.LJMD_ERR_INVALID_ARG and "every" in msg
        code, msg = _err(eng.heatflux_accumulate)                                   # before configure
        assert code == _lib.LJMD_ERR_STATE and "ljmd_batch_heatflux_configure first" in msg
        eng.heatflux_configure(2)
        # the pressure tensor's guard is its own (the order of the two inside one call: tests/batch_heatflux_host)
        assert lib.ljmd_batch_stress_accumulate(eng._h) == _lib.LJMD_ERR_STATE
        assert "ljmd_batch_stress_configure first" in _lib.batch_last_error(eng._h)
        code, msg = _err(lambda: eng.heatflux_configure(-3))                        # a failed guard keeps the configuration
        assert code == _lib.LJMD_ERR_INVALID_ARG and eng.heatflux_read_exact().shape == (0, B, 9)
        code, msg = _err(eng.heatflux_accumulate)                                   # configured, then: before a state
        assert code == _lib.LJMD_ERR_STATE and "no state" in msg
        bad = r.copy()
        bad[1, :, 1] = bad[1, :, 0]
        bad[1, 0, 1] += 0.05                                                        # the reproducible force pass fails ...
        _set(eng, bad, v)
        assert _err(eng.compute_forces)[0] == _lib.LJMD_ERR_RANGE
        code, msg = _err(eng.heatflux_accumulate)                                   # ... and poisons the handle
        assert code == _lib.LJMD_ERR_STATE and "poisoned" in msg
        assert eng.heatflux_read_exact().shape == (0, B, 9)                         # a poisoned handle may still be read
        eng.heatflux_configure(0)                                                   # not configured comes before poisoned
        code, msg = _err(eng.heatflux_accumulate)
        assert code == _lib.LJMD_ERR_STATE and "ljmd_batch_heatflux_configure first" in msg
        eng.heatflux_configure(2)
        _set(eng, r, v)
        eng.heatflux_accumulate()
        assert eng.heatflux_read_exact().shape == (1, B, 9)
