"""-m gpu: the density modes rho_k of every replica recorded on the device by the batch engine (ljmd_batch_rhok_*,
BatchEngine.rhok_*).  A snapshot of a replica is two exact integers per mode: every comparison of words is equality
with tests/rhok_model.py (numpy arithmetic, Python ints) on the state get_state returns, or with the single engine's
ljmd_rhok_* given the same state.  The kernel gives a workgroup one replica and 64 modes, its waves the replica's tiles
of 64 particles: the particle numbers straddle the tile and the kernel classes, the mode lists the 64."""
import functools

import numpy as np
import pytest

import rhok_model
from ljmd_amd import BatchEngine, Engine, _lib, analysis, md_types, synthetic
from ljmd_amd._lib import LjmdError

pytestmark = pytest.mark.gpu

REPRO = _lib.PRECISION_FP64_REPRODUCIBLE
SPECIAL = [(0, 0, 0), (1, 0, 0), (-1, 0, 0), (-3, 2, 7), (3, -2, -7), (1023, -1023, 1023), (1, 0, 0), (-1023, 1023, -1023)]


def _mode_list(count, seed=0):
    """`count` triples: (0, 0, 0), negatives, a duplicate and the index limit first, then random ones up to |n_a| = 40"""
    rng = np.random.default_rng(100 + count + seed)
    rest = rng.integers(-40, 41, size=(max(count - len(SPECIAL), 0), 3))
    return np.concatenate([np.array(SPECIAL), rest])[:count].astype(np.int32)


def _config(n, seed, rho=0.8):
    """-> (params, r [3, n], v [3, n]); n = 1, the smallest system the batch engine accepts, has no lattice of its own"""
    if n == 1:
        rng = np.random.Generator(np.random.PCG64(seed))
        return md_types.init_params(1, 4.0, 0.005, 1.9), 4.0 * rng.random((3, 1)), np.zeros((3, 1))
    return synthetic.make_config(n, seed=seed, rho=rho)


def _replicas(n, seeds, rho=0.8):
    cfg = [_config(n, s, rho) for s in seeds]
    return cfg[0][0], np.stack([c[1] for c in cfg]), np.stack([c[2] for c in cfg])       # p, r[B, 3, n], v[B, 3, n]


def _set(eng, r, v):
    eng.set_state(r[:, 0], r[:, 1], r[:, 2], v[:, 0], v[:, 1], v[:, 2])


def _set_per_replica(eng, cfg):
    eng.set_state(*[[c[1][ax] for c in cfg] for ax in range(3)], *[[c[2][ax] for c in cfg] for ax in range(3)])


def _r(eng):
    """-> per replica r [3, n_b] of the resident state; works for both kinds of engine"""
    st = eng.get_state(("r",))
    return [np.stack([np.asarray(st["r"][ax][b]) for ax in range(3)]) for b in range(eng.n_replicas)]


def _flat_state(eng):
    st = eng.get_state()
    return [np.concatenate([np.ravel(x) for x in st[key][ax]]) for key in ("r", "ru", "v", "a") for ax in range(3)]


def _one_shot(eng, modes):
    """configure, one accumulate -> words[B][n_modes] as [Re, Im] lists"""
    eng.rhok_configure(modes, 1)
    eng.rhok_accumulate()
    words = eng.rhok_read_exact()
    assert words.shape == (1, eng.n_replicas, len(modes), 2)
    return [[list(w) for w in words[0, b]] for b in range(eng.n_replicas)]


def _model(rb, L, modes):
    want, flag = rhok_model.words(rb, L, modes)
    assert not flag
    return want


def _err(call):
    with pytest.raises(LjmdError) as ei:
        call()
    return ei.value.code, ei.value.message


# ---- 1. one-shot words -----------------------------------------------------------------------------------------------
# n: the smallest system; 63, 64, 65: one short of a tile, one tile, one beyond; 128 | 129, 512, 1025, 2048, 4096: the
# borders of the five kernel classes; 4096: 64 tiles, 8 per wave, the most a wave gets.  1, 63, 64, 65, 257 modes: below,
# at and beyond one and four mode chunks.  Every n with 65 modes, every mode count with the smallest and the largest n.
# Only positions are set: no forces are needed.
SHAPES = [(n, 65) for n in (1, 63, 64, 65, 128, 129, 512, 1025, 2048, 4096)] + \
         [(1, 1), (1, 63), (1, 64), (1, 257), (63, 64), (64, 63), (65, 1), (128, 257), (129, 64), (512, 63), (1025, 257),
          (2048, 1), (4096, 1), (4096, 63), (4096, 64), (4096, 257)]


@pytest.mark.parametrize("n, count", SHAPES)
def test_one_shot_words_equal_the_model(n, count):
    B = 3
    p, r, v = _replicas(n, range(600, 600 + B))
    modes = _mode_list(count)
    with BatchEngine(p, B) as eng:
        _set(eng, r, v)
        got = _one_shot(eng, modes)
        raw = eng.rhok_read_exact(raw=True)
        rho = eng.rhok_read()
        state = _r(eng)
        assert eng.rhok_profile()["kernel_ms"] > 0.0
    assert raw.shape == (1, B, count, 2, 3) and rho.shape == (1, B, count) and rho.dtype == np.complex128
    for b in range(B):
        assert state[b].tobytes() == r[b].tobytes()
        want = _model(state[b], p.box_length, modes)
        assert got[b] == want, (b, [tuple(modes[m]) for m in range(count) if got[b][m] != want[m]])
        assert got[b][0] == [n << 64, 0]                            # (0, 0, 0): every particle once, nothing else
        assert raw[0, b].tolist() == [[rhok_model.to_limbs(x) for x in w] for w in want]
        assert rho[0, b].tobytes() == rhok_model.doubles(want).tobytes()
        for m in range(count):
            for k in range(m + 1, count):
                if (modes[m] == -modes[k]).all():
                    assert got[b][k] == [got[b][m][0], -got[b][m][1]]   # mode -n is the exact conjugate
        if count >= 7:
            assert got[b][6] == got[b][1] and got[b][1][1] != 0    # the duplicate
    if count > 1:
        assert got[1] != got[0] and got[2] != got[0]                # each row is its own replica's


@pytest.mark.parametrize("waves", ["2", "4", "8"])
def test_every_wave_count_of_the_kernel(monkeypatch, waves):
    """LJMD_BATCH_RHOK_WAVES (read by configure) reaches the kernel's variants of 2 and 4 waves per workgroup, which exist
    for tools/batch_rhok_rate.py beside the 8 that are launched otherwise: the same words.  n = 65 leaves waves without a
    tile, 1025 a ragged last tile, 4096 gives a wave of the 2-wave variant 32 tiles"""
    monkeypatch.setenv("LJMD_BATCH_RHOK_WAVES", waves)
    modes = _mode_list(65)
    for n in (65, 1025, 4096):
        p, r, v = _replicas(n, [611, 612])
        with BatchEngine(p, 2) as eng:
            _set(eng, r, v)
            got = _one_shot(eng, modes)
        for b in range(2):
            assert got[b] == _model(r[b], p.box_length, modes), (n, b)


# ---- 2. mixed replicas in one call -----------------------------------------------------------------------------------
MIX = [(65, 0.60, 31), (4096, 0.75, 36), (108, 0.80, 32), (500, 0.95, 33), (1025, 0.70, 34), (1000, 0.65, 39), (2049, 0.85, 37),
       (1, 0.8, 38), (108, 0.85, 35)]     # (n, rho, seed): all five classes, nine different L, the classes not in table order


def _mix_cfg():
    return [_config(n, s, rho) for n, rho, s in MIX]


def _batch_class(n):
    """the kernel class of a replica of n particles (csrc/ljmd_batch.h: batch_class)"""
    return 0 if n <= 128 else 1 if n <= 512 else 2 if n <= 1024 else 3 if n <= 2048 else 4


@functools.lru_cache(maxsize=None)
def _mix_model(count):
    return [_model(c[1], c[0].box_length, _mode_list(count)) for c in _mix_cfg()]


@pytest.mark.parametrize("streams", ["1", "0"])
def test_mixed_replicas_in_one_call(monkeypatch, streams):
    """each replica's words are the model's for its own n_b and L_b, with the groups on streams of their own and one after
    another on the handle's"""
    monkeypatch.setenv("LJMD_BATCH_GROUP_STREAMS", streams)
    cfg = _mix_cfg()
    assert {_batch_class(c[0].n) for c in cfg} == {0, 1, 2, 3, 4}
    modes = _mode_list(65)
    with BatchEngine.per_replica([c[0] for c in cfg]) as eng:
        _set_per_replica(eng, cfg)
        got = _one_shot(eng, modes)
    want = _mix_model(65)
    for b in range(len(cfg)):
        assert got[b] == want[b], b


# ---- 3. the same integers as the single engine -----------------------------------------------------------------------
@pytest.mark.parametrize("n", [108, 4096])
def test_same_integers_as_the_single_engine(n):
    B = 2
    p, r, v = _replicas(n, range(620, 620 + B))
    modes = _mode_list(129)
    with BatchEngine(p, B) as eng:
        _set(eng, r, v)
        got = _one_shot(eng, modes)
        raw = eng.rhok_read_exact(raw=True)
    for b in range(B):
        with Engine(p) as one:
            one.set_state(r[b, 0], r[b, 1], r[b, 2], v[b, 0], v[b, 1], v[b, 2])
            one.rhok_configure(modes, 1)
            one.rhok_accumulate()
            assert one.rhok_read_exact(raw=True)[0].tolist() == raw[0, b].tolist(), b
            assert [list(w) for w in one.rhok_read_exact()[0]] == got[b]


# ---- 4. a replica's words are its own --------------------------------------------------------------------------------
def test_words_do_not_depend_on_batch_size_or_slot():
    n = 108
    p, r, v = _replicas(n, range(640, 640 + 64))
    modes = _mode_list(65)
    got = {}
    for B, slot in ((1, 0), (3, 2), (64, 37), (64, 0)):
        rr, vv = r[:B].copy(), v[:B].copy()
        rr[[0, slot]], vv[[0, slot]] = rr[[slot, 0]], vv[[slot, 0]]      # configuration 0 sits in `slot`
        with BatchEngine(p, B) as eng:
            _set(eng, rr, vv)
            got[B, slot] = _one_shot(eng, modes)[slot]
    assert got[1, 0] == _model(r[0], p.box_length, modes)
    for key, w in got.items():
        assert w == got[1, 0], key


def test_words_do_not_depend_on_neighbours_particle_order_or_precision_mode():
    cfg = _mix_cfg()
    modes = _mode_list(65)
    want = _mix_model(65)

    def run(c, mode=_lib.PRECISION_FP64):
        with BatchEngine.per_replica([x[0] for x in c], precision_mode=mode) as eng:
            _set_per_replica(eng, c)
            return _one_shot(eng, modes)

    rev = run(cfg[::-1])
    for b in range(len(cfg)):
        assert rev[len(cfg) - 1 - b] == want[b], b
    assert run([cfg[3]]) == [want[3]]                               # alone
    perm = np.random.Generator(np.random.PCG64(5)).permutation(cfg[3][0].n)
    shuffled = cfg[:3] + [(cfg[3][0], cfg[3][1][:, perm], cfg[3][2][:, perm])] + cfg[4:]
    assert run(shuffled) == want                                    # an integer sum does not see the order
    assert run(cfg, REPRO) == want                                  # the same positions in the reproducible mode
    with BatchEngine.per_replica([x[0] for x in cfg]) as eng:       # ... and after a change of mode on one handle
        _set_per_replica(eng, cfg)
        eng.set_precision(REPRO)
        _set_per_replica(eng, cfg)
        assert _one_shot(eng, modes) == want


def test_mode_list_independence():
    """mode m's words are the same in any list: permuted, alone, with duplicates, and in the longest list"""
    n, B = 500, 2
    p, r, v = _replicas(n, [661, 662])
    rng = np.random.default_rng(8)
    big = np.concatenate([_mode_list(257), rng.integers(-1023, 1024, size=(_lib.RHOK_MAX_MODES - 257, 3))]).astype(np.int32)
    perm = rng.permutation(257)
    with BatchEngine(p, B) as eng:
        _set(eng, r, v)
        base = _one_shot(eng, big[:257])
        permuted = _one_shot(eng, big[:257][perm])
        alone = _one_shot(eng, big[3:4])
        doubled = _one_shot(eng, np.concatenate([big[:70], big[:70]]))
        full = _one_shot(eng, big)
    for b in range(B):
        assert base[b] == _model(r[b], p.box_length, big[:257])
        assert permuted[b] == [base[b][k] for k in perm]
        assert alone[b] == [base[b][3]]
        assert doubled[b] == base[b][:70] + base[b][:70]
        assert full[b][:257] == base[b]
        pick = list(range(257, _lib.RHOK_MAX_MODES, 197)) + [_lib.RHOK_MAX_MODES - 1]
        assert [full[b][m] for m in pick] == _model(r[b], p.box_length, big[pick])


# ---- 5. symmetry -----------------------------------------------------------------------------------------------------
def test_conjugate_modes_and_the_zero_mode():
    cfg = _mix_cfg()
    rng = np.random.default_rng(9)
    half = rng.integers(-1023, 1024, size=(100, 3)).astype(np.int32)
    modes = np.concatenate([np.zeros((1, 3), dtype=np.int32), half, -half])
    with BatchEngine.per_replica([c[0] for c in cfg]) as eng:
        _set_per_replica(eng, cfg)
        got = _one_shot(eng, modes)
    for b, c in enumerate(cfg):
        assert got[b][0] == [c[0].n << 64, 0]
        for m in range(1, 101):
            assert got[b][100 + m] == [got[b][m][0], -got[b][m][1]], (b, m)
        assert any(got[b][m][1] != 0 for m in range(1, 101))


# ---- 6. snapshots taken inside steps() -------------------------------------------------------------------------------
SWEEP = [(108, 0.80, 21), (500, 0.60, 22), (108, 0.95, 23), (1372, 0.70, 24)]     # (n, rho, seed): three kernel classes
STEPS, SAMPLE, NBINS = 12, 4, 60
MODES6 = 70


def _started(cfg, mode=REPRO):
    eng = BatchEngine.per_replica([c[0] for c in cfg], precision_mode=mode)
    _set_per_replica(eng, cfg)
    eng.compute_forces()
    return eng


def _configure_others(eng):
    eng.rdf_configure(NBINS, every=3)
    eng.tcf_configure(4, 1, every=2)
    eng.stress_configure(4, every=12)
    eng.heatflux_configure(8, every=4)
    eng.vanhove_configure(4, 1, 16, every=3)


def _read_others(eng):
    return eng.rdf_read(), eng.tcf_read_exact(), eng.stress_read_exact(), eng.heatflux_read_exact(), eng.vanhove_read_exact()


def _same(a, b):
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return np.array_equal(a, b)


@pytest.fixture(scope="module")
def sweep_reference():
    """computed once, in the reproducible mode, on handles without the density modes: the model's words on the state a
    second run stopped at steps 2, 4, .. returns, scalars and final state of a plain run, and the other five observables
    of a run that has them alone"""
    cfg = [synthetic.make_config(n, seed=s, rho=rho) for n, rho, s in SWEEP]
    modes = _mode_list(MODES6)
    model = {}
    for step in (4, 6, 8, 12):
        with _started(cfg) as eng:
            eng.steps(step, observables=False)                      # a run stopped at this step
            model[step] = [_model(rb, cfg[b][0].box_length, modes) for b, rb in enumerate(_r(eng))]
    with _started(cfg) as eng:
        plain = (eng.steps(STEPS, SAMPLE), _flat_state(eng))
    with _started(cfg) as eng:
        _configure_others(eng)
        eng.steps(STEPS, SAMPLE)
        others = _read_others(eng)
    return cfg, modes, model, plain, others


@pytest.mark.parametrize("streams, every, with_others", [("1", 4, False), ("0", 6, False), ("1", 6, True), ("0", 4, True)])
def test_snapshots_inside_steps(sweep_reference, monkeypatch, streams, every, with_others):
    cfg, modes, model, (want_scalars, want_state), want_others = sweep_reference
    monkeypatch.setenv("LJMD_BATCH_GROUP_STREAMS", streams)
    rows = STEPS // every
    with _started(cfg) as eng:
        eng.rhok_configure(modes, rows + 1, every=every)
        if with_others:
            _configure_others(eng)
        scalars = eng.steps(STEPS, SAMPLE)
        prof = eng.profile_read()
        words = eng.rhok_read_exact()
        state = _flat_state(eng)
        if with_others:
            assert _same(_read_others(eng), want_others)
        else:
            code, msg = _err(lambda: eng.steps(every + 1, observables=False))   # not a multiple: refused, nothing launched
            assert code == _lib.LJMD_ERR_INVALID_ARG
            assert "density modes interval %d (ljmd_batch_rhok_configure: every)" % every in msg
            assert eng.rhok_read_exact().shape == (rows, len(cfg), MODES6, 2)
            assert [a.tobytes() for a in _flat_state(eng)] == [a.tobytes() for a in state]
    assert words.shape == (rows, len(cfg), MODES6, 2)
    for k in range(rows):
        for b in range(len(cfg)):
            assert [list(w) for w in words[k, b]] == model[(k + 1) * every][b], (k, b)
    for got, ref in zip(scalars, want_scalars):
        assert got.shape == ref.shape and got.tobytes() == ref.tobytes()
    for got, ref in zip(state, want_state):
        assert got.tobytes() == ref.tobytes()
    # three kernel classes, each with its step launches split at the snapshots and one density modes launch per snapshot
    assert prof["launches"] >= 3 * 2 * rows and prof["kernel_ms"] > 0.0, prof


# ---- 7. accumulating leaves everything else bitwise alone ------------------------------------------------------------
@pytest.mark.parametrize("mode", [_lib.PRECISION_FP64, REPRO])
def test_accumulating_leaves_everything_else_alone(mode):
    cfg = [synthetic.make_config(n, seed=s, rho=rho) for n, rho, s in SWEEP]
    modes = _mode_list(MODES6)
    out = {}
    for on in (False, True):
        with _started(cfg, mode) as eng:
            _configure_others(eng)
            if on:
                eng.rhok_configure(modes, 16, every=2)
                eng.rhok_accumulate()
            first = eng.steps(STEPS, SAMPLE)
            if on:
                eng.rhok_accumulate()
                eng.rhok_accumulate()
            second = eng.steps(STEPS, 1)
            out[on] = (first, second, _flat_state(eng), _read_others(eng))
            if on:
                assert eng.rhok_read_exact().shape[0] == 3 + 2 * (STEPS // 2)
    for got, ref in zip(out[True][0] + out[True][1], out[False][0] + out[False][1]):
        assert got.tobytes() == ref.tobytes()
    assert [a.tobytes() for a in out[True][2]] == [a.tobytes() for a in out[False][2]]
    assert _same(out[True][3], out[False][3])


# ---- 8. positions spanning several boxes -----------------------------------------------------------------------------
def test_raw_coordinates_three_boxes_away():
    """the replicas sit 3 L and -3 L away from the box along different axes; the words are the model's on those raw
    coordinates, and (0, 0, 0) still counts every particle"""
    n, B = 500, 3
    p, r, v = _replicas(n, [671, 672, 673])
    L = p.box_length
    far = r.copy()
    far[0] += (3.0 * L * np.array([1.0, -1.0, 0.0]))[:, None]
    far[1] += (3.0 * L * np.array([-1.0, 1.0, 1.0]))[:, None]
    far[2, 2] -= 3.0 * L
    modes = _mode_list(129)
    with BatchEngine(p, B) as eng:
        _set(eng, far, v)
        got = _one_shot(eng, modes)
        state = _r(eng)
    for b in range(B):
        assert state[b].tobytes() == far[b].tobytes()
        assert np.abs(far[b]).max() > 2.9 * L
        assert got[b] == _model(far[b], L, modes), b
        assert got[b][0] == [n << 64, 0]


# ---- 9. a NaN coordinate in one replica ------------------------------------------------------------------------------
def test_a_nan_coordinate_sets_the_replicas_sticky_word():
    """ljmd_batch_set_state refuses a position that is not finite, so the NaN arrives the way it would in a run: one
    acceleration component of replica 1 is NaN and the next step carries it into r.  An arithmetic flag: nothing faults"""
    n, B = 108, 3
    p, r, v = _replicas(n, [681, 682, 683])
    modes = _mode_list(65)
    lib = _lib.load()
    with BatchEngine(p, B) as eng, BatchEngine(p, B) as plain:
        for e in (eng, plain):
            _set(e, r, v)
            e.compute_forces()
            ay = np.stack(e.get_state(("a",))["a"][1])
            ay[1, 7] = np.nan
            e.set_accel(None, ay, None)
        eng.rhok_configure(modes, 4)
        got_steps, ref_steps = eng.steps(1, 1), plain.steps(1, 1)
        eng.rhok_accumulate()
        state = _r(eng)
        assert [int(np.isnan(s).sum()) > 0 for s in state] == [False, True, False] and np.isnan(state[1][1, 7])
        for read in (eng.rhok_read, eng.rhok_read_exact):
            code, msg = _err(read)
            assert code == _lib.LJMD_ERR_RANGE and "replica 1" in msg and "ljmd_batch_rhok_reset" in msg, msg
        # read_exact has delivered the words all the same: every row is the model's, the flagged replica's terms as zeros
        raw = np.zeros((4, B, 65, 2, 3), dtype=np.int64)
        assert lib.ljmd_batch_rhok_read_exact(eng._h, raw.ctypes.data_as(_lib.c_int64_p), None) == _lib.LJMD_ERR_RANGE
        for b in range(B):
            want, flag = rhok_model.words(state[b], p.box_length, modes)
            assert flag == (b == 1)
            assert raw[0, b].tolist() == [[rhok_model.to_limbs(x) for x in w] for w in want], b
        bad_live = int(np.isfinite(state[1]).all(axis=0).sum())
        assert bad_live < n and raw[0, 1, 0].tolist() == [rhok_model.to_limbs(bad_live << 64), [0, 0, 0]]
        # stepping is unaffected, and the handle is not poisoned
        for a, c in zip(got_steps + eng.steps(2, 1), ref_steps + plain.steps(2, 1)):
            assert a.tobytes() == c.tobytes()
        assert [a.tobytes() for a in _flat_state(eng)] == [a.tobytes() for a in _flat_state(plain)]
        assert _err(eng.rhok_read_exact)[0] == _lib.LJMD_ERR_RANGE              # sticky until reset
        # the NaN removed: after reset and a new accumulate every replica's words are the model's
        clean = np.stack(state)
        clean[1] = r[1]
        _set(eng, clean, v)
        assert _err(eng.rhok_read_exact)[0] == _lib.LJMD_ERR_RANGE              # set_state keeps the word
        eng.rhok_reset()
        assert eng.rhok_read_exact().shape == (0, B, 65, 2)
        eng.rhok_accumulate()
        words = eng.rhok_read_exact()
        for b in range(B):
            assert [list(w) for w in words[0, b]] == _model(clean[b], p.box_length, modes), b


# ---- 10. bookkeeping and guards, in order ----------------------------------------------------------------------------
def test_bookkeeping_and_guards_in_order():
    n, B = 108, 3
    p, r, v = _replicas(n, [691, 692, 693])
    modes = _mode_list(10)
    mp = modes.ctypes.data_as(_lib.c_int32_p)
    lib = _lib.load()
    # a NULL handle comes first, whatever the other arguments
    for call in (lambda: lib.ljmd_batch_rhok_configure(None, -1, None, -1, -1), lambda: lib.ljmd_batch_rhok_accumulate(None),
                 lambda: lib.ljmd_batch_rhok_read_exact(None, None, None), lambda: lib.ljmd_batch_rhok_read(None, None, None),
                 lambda: lib.ljmd_batch_rhok_reset(None), lambda: lib.ljmd_batch_rhok_profile_read(None, None)):
        assert call() == _lib.LJMD_ERR_INVALID_ARG and "NULL handle" in _lib.batch_last_error()
    with BatchEngine(p, B, precision_mode=REPRO) as eng:
        # not configured
        for call in (eng.rhok_accumulate, eng.rhok_read, eng.rhok_read_exact, eng.rhok_reset, eng.rhok_profile):
            code, msg = _err(call)
            assert code == _lib.LJMD_ERR_STATE and "ljmd_batch_rhok_configure first" in msg
        # configure's guards: max_snapshots, every, then the mode rules, then the entry cap
        for bad in (-1, _lib.BATCH_RHOK_MAX_SNAPSHOTS + 1):
            code, msg = _err(lambda: eng.rhok_configure(modes, bad, -1))
            assert code == _lib.LJMD_ERR_INVALID_ARG and msg.startswith("ljmd_batch_rhok_configure: max_snapshots"), msg
        code, msg = _err(lambda: eng.rhok_configure(modes, 2, -1))
        assert code == _lib.LJMD_ERR_INVALID_ARG and "every" in msg
        assert lib.ljmd_batch_rhok_configure(eng._h, 0, mp, 2, 0) == _lib.LJMD_ERR_INVALID_ARG
        assert "n_modes = 0 outside 1..4096" in _lib.batch_last_error(eng._h)
        assert lib.ljmd_batch_rhok_configure(eng._h, _lib.RHOK_MAX_MODES + 1, mp, 2, 0) == _lib.LJMD_ERR_INVALID_ARG
        assert lib.ljmd_batch_rhok_configure(eng._h, 10, None, 2, 0) == _lib.LJMD_ERR_INVALID_ARG
        assert "modes is NULL" in _lib.batch_last_error(eng._h)
        for tr in ((1024, 0, 0), (0, -1024, 0), (0, 0, 1 << 20)):
            badm = modes.copy()
            badm[4] = tr
            code, msg = _err(lambda: eng.rhok_configure(badm, _lib.BATCH_RHOK_MAX_SNAPSHOTS))   # triples before the cap
            assert code == _lib.LJMD_ERR_INVALID_ARG and "mode 4 = " in msg and "outside -1023..1023" in msg, msg
        edge = np.array([[1023, -1023, 0]], dtype=np.int32)
        longest = np.ones((_lib.RHOK_MAX_MODES, 3), dtype=np.int32)
        cap = _lib.BATCH_RHOK_MAX_ENTRIES // (B * _lib.RHOK_MAX_MODES)                   # 1365 snapshots of 3 x 4096 modes
        assert cap < _lib.BATCH_RHOK_MAX_SNAPSHOTS
        code, msg = _err(lambda: eng.rhok_configure(longest, cap + 1))                   # the entry cap counts B
        assert code == _lib.LJMD_ERR_INVALID_ARG and "max_snapshots * B * n_modes" in msg, msg
        assert _err(eng.rhok_accumulate)[0] == _lib.LJMD_ERR_STATE                       # still not configured
        eng.rhok_configure(edge, 2)
        assert eng.rhok_read_exact().shape == (0, B, 1, 2) and eng.rhok_read().shape == (0, B, 1)
        assert eng.rhok_profile() == {"kernel_ms": 0.0}
        code, msg = _err(lambda: eng.rhok_configure(modes, -3))                          # a failed guard keeps the configuration
        assert code == _lib.LJMD_ERR_INVALID_ARG and eng.rhok_read_exact().shape == (0, B, 1, 2)
        # another observable's guard is its own
        assert lib.ljmd_batch_vanhove_accumulate(eng._h) == _lib.LJMD_ERR_STATE
        assert "ljmd_batch_vanhove_configure first" in _lib.batch_last_error(eng._h)
        # no state
        code, msg = _err(eng.rhok_accumulate)
        assert code == _lib.LJMD_ERR_STATE and "no state" in msg
        # a poisoned handle: the reproducible force pass fails on two particles that all but coincide
        eng.rhok_configure(modes, 3)
        _set(eng, r, v)
        eng.rhok_accumulate()                                                            # needs no accelerations
        bad = r.copy()
        bad[1, :, 1] = bad[1, :, 0]
        bad[1, 0, 1] += 0.05
        _set(eng, bad, v)
        assert _err(eng.compute_forces)[0] == _lib.LJMD_ERR_RANGE
        code, msg = _err(eng.rhok_accumulate)
        assert code == _lib.LJMD_ERR_STATE and "poisoned" in msg
        kept = eng.rhok_read_exact()                                                     # ... which may still be read
        assert kept.shape == (1, B, 10, 2) and eng.rhok_read().shape == (1, B, 10)
        eng.rhok_reset()                                                                 # ... and reset
        _set(eng, r, v)                                                                  # set_state heals
        eng.compute_forces()
        # a full series
        for _ in range(3):
            eng.rhok_accumulate()
        code, msg = _err(eng.rhok_accumulate)
        assert code == _lib.LJMD_ERR_STATE and "full" in msg and "ljmd_batch_rhok_reset" in msg
        full = eng.rhok_read_exact()
        assert full.shape == (3, B, 10, 2) and np.array_equal(full[0], full[2]) and np.array_equal(full[0], kept[0])
        for b in range(B):
            assert [list(w) for w in full[0, b]] == _model(r[b], p.box_length, modes)
        assert lib.ljmd_batch_rhok_read(eng._h, None, None) == _lib.LJMD_OK             # every pointer may be NULL
        assert lib.ljmd_batch_rhok_read_exact(eng._h, None, None) == _lib.LJMD_OK
        assert lib.ljmd_batch_rhok_profile_read(eng._h, None) == _lib.LJMD_OK
        # every: not dividing nsteps, then the room check, both before anything is launched
        eng.rhok_configure(modes, 3, every=2)                                            # a reconfigure frees and starts over
        assert eng.rhok_read_exact().shape == (0, B, 10, 2)
        before = [a.tobytes() for a in _flat_state(eng)]
        code, msg = _err(lambda: eng.steps(3, observables=False))
        assert code == _lib.LJMD_ERR_INVALID_ARG and "is not a multiple of the density modes interval 2" in msg, msg
        code, msg = _err(lambda: eng.steps(8, observables=False))                        # 4 snapshots, room for 3
        assert code == _lib.LJMD_ERR_STATE and "full" in msg
        assert [a.tobytes() for a in _flat_state(eng)] == before and eng.rhok_read_exact().shape[0] == 0
        eng.steps(6, observables=False)
        three = eng.rhok_read_exact()
        assert three.shape == (3, B, 10, 2) and not np.array_equal(three[0], three[2])
        assert _err(lambda: eng.steps(2, observables=False))[0] == _lib.LJMD_ERR_STATE
        # set_state and the other setters keep the series
        _set(eng, r[::-1].copy(), v[::-1].copy())
        eng.set_precision(_lib.PRECISION_FP64)
        eng.set_precision(REPRO)
        _set(eng, r, v)
        eng.set_tail_corrections(False)
        eng.rdf_configure(20)
        eng.vanhove_configure(4)
        assert np.array_equal(eng.rhok_read_exact(), three)
        eng.rhok_reset()
        eng.prepare([5, 6, 7], -500.0, warmup_steps=4)                                   # the warm-up takes no snapshot
        assert eng.rhok_read_exact().shape[0] == 0
        eng.steps(2, observables=False)                                                  # ... and the interval is back
        one = eng.rhok_read_exact()
        assert one.shape[0] == 1
        for b, rb in enumerate(_r(eng)):
            assert [list(w) for w in one[0, b]] == _model(rb, p.box_length, modes), b
        # max_snapshots = 0 switches the feature off, whatever the other arguments
        assert lib.ljmd_batch_rhok_configure(eng._h, -5, None, 0, 0) == _lib.LJMD_OK
        for call in (lambda: lib.ljmd_batch_rhok_accumulate(eng._h), lambda: lib.ljmd_batch_rhok_reset(eng._h),
                     lambda: lib.ljmd_batch_rhok_read(eng._h, None, None),
                     lambda: lib.ljmd_batch_rhok_read_exact(eng._h, None, None)):
            assert call() == _lib.LJMD_ERR_STATE
            assert "ljmd_batch_rhok_configure first" in _lib.batch_last_error(eng._h)
        eng.steps(3, observables=False)                                                  # today's stepping
        eng.rhok_configure(modes, 5, every=1)                                            # destroyed while configured
        eng.steps(2, observables=False)


def test_python_argument_checks():
    p, r, v = _replicas(108, [695])
    with BatchEngine(p, 1) as eng:
        with pytest.raises(TypeError):
            eng.rhok_configure(_mode_list(3), 2.0)
        with pytest.raises(TypeError):
            eng.rhok_configure(_mode_list(3), 2, every=True)
        with pytest.raises(TypeError):
            eng.rhok_configure(np.zeros((3, 3)), 2)
        with pytest.raises(ValueError):
            eng.rhok_configure(np.zeros((3, 2), dtype=np.int32), 2)


# ---- 11. the ensemble functions --------------------------------------------------------------------------------------
def test_ensemble_functions_on_a_jittered_lattice():
    """B = 4 replicas of a jittered simple cubic lattice of 8^3 particles, three snapshots a few steps apart: per replica
    the ensemble functions return exactly what the single-system functions return for rho[:, b]; the Bragg shell |n|^2 =
    64 stands out of the first shell in the ensemble mean"""
    n, B = 512, 4
    p, r, v = _replicas(n, [701, 702, 703, 704])
    L = p.box_length
    modes = np.array([(1, 0, 0), (0, 1, 0), (0, 0, 1), (8, 0, 0), (0, 8, 0), (0, 0, 8)], dtype=np.int32)
    with BatchEngine(p, B) as eng:
        _set(eng, r, v)
        eng.compute_forces()
        eng.rhok_configure(modes, 3, every=2)
        eng.rhok_accumulate()
        eng.steps(4, observables=False)
        rho = eng.rhok_read()
    assert rho.shape == (3, B, 6)
    per, mean, err = analysis.static_structure_factor_ensemble(rho, n, modes, L)
    fper, fmean, ferr = analysis.intermediate_scattering_ensemble(rho, n, modes, 2, 1)
    assert len(per) == B and fper.shape == (B, 2, 3)
    for b in range(B):
        one = analysis.static_structure_factor(rho[:, b], n, modes, L)
        assert all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(per[b], one))
        assert fper[b].tobytes() == analysis.intermediate_scattering(rho[:, b], n, modes, 2, 1).tobytes()
    S = np.stack([q[1] for q in per])
    assert mean.tobytes() == S.mean(axis=0).tobytes() and err.tobytes() == (S.std(axis=0, ddof=1) / 2.0).tobytes()
    assert fmean.tobytes() == fper.mean(axis=0).tobytes() and ferr.tobytes() == (fper.std(axis=0, ddof=1) / 2.0).tobytes()
    assert 0.5 * n < mean[1] < n and mean[0] < 2.0, mean
    assert (err > 0.0).all() and (err < mean + 1.0).all()
