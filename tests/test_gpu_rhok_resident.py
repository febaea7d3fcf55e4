"""-m gpu: the collective density modes of the resident system recorded on the one-rank engine (ljmd_rhok_*,
Engine.rhok_*).  A snapshot is two exact integers per mode: every comparison of words is equality with
tests/rhok_model.py (numpy arithmetic, Python ints) on the state get_state returns.  The terms kernel gives a wave 64
modes and a chunk of whole 64-slot tiles; the mode lists straddle the 64, the particle numbers the tile."""
import functools

import numpy as np
import pytest

import rhok_model
from ljmd_amd import Engine, _lib, analysis, md_types, synthetic
from ljmd_amd._lib import LjmdError

pytestmark = pytest.mark.gpu

REPRO = _lib.PRECISION_FP64_REPRODUCIBLE
PRECISIONS = {"fp64": _lib.PRECISION_FP64, "mixed": _lib.PRECISION_FP32_FORCE, "reproducible": REPRO}
SPECIAL = [(0, 0, 0), (1, 0, 0), (-1, 0, 0), (-3, 2, 7), (3, -2, -7), (1023, -1023, 1023), (1, 0, 0), (-1023, 1023, -1023)]


def _mode_list(count, seed=0):
    """`count` triples: (0, 0, 0), negatives, a duplicate and the index limit first, then random ones up to |n_a| = 40"""
    rng = np.random.default_rng(100 + count + seed)
    rest = rng.integers(-40, 41, size=(max(count - len(SPECIAL), 0), 3))
    return np.concatenate([np.array(SPECIAL), rest])[:count].astype(np.int32)


def _params(n, seed=None, rho=0.8):
    p, r, v = synthetic.make_config(n, seed=1000 + n if seed is None else seed, rho=rho)
    return md_types.init_params(n, p.box_length, p.dt, min(2.5, 0.49 * p.box_length)), r, v


def _r(eng):
    return np.stack(eng.get_state(("r",))["r"])


def _one_shot(eng, modes, max_snapshots=1):
    """configure, one accumulate -> [[Re, Im] per mode]"""
    eng.rhok_configure(modes, max_snapshots)
    eng.rhok_accumulate()
    words = eng.rhok_read_exact()
    assert words.shape == (1, len(modes), 2)
    return [list(w) for w in words[0]]


@functools.lru_cache(maxsize=None)
def _initial_model(n, count):
    p, r, _v = _params(n)
    return rhok_model.words(r, p.box_length, _mode_list(count))


# ---- 1. one-shot words -----------------------------------------------------------------------------------------------
# n = 108, 500: the gather engine, a partly filled last tile.  n = 4096: full tiles; n = 4100: 4 live lanes in the 65th
# tile; n = 63, 65: one slot short of a tile and one beyond (a tile is the particle chunk of these sizes).  1, 63, 64,
# 65, 257 modes: below, at and beyond one and four mode chunks.  Only positions are set: no forces are needed.
@pytest.mark.parametrize("n, count", [(108, 1), (108, 65), (500, 63), (500, 257), (4096, 64), (4096, 257), (4100, 65),
                                      (4100, 1), (63, 64), (65, 65)])
def test_one_shot_words_equal_the_model(n, count):
    p, r, v = _params(n)
    modes = _mode_list(count)
    with Engine(p) as eng:
        eng.set_state(r[0], r[1], r[2], v[0], v[1], v[2])
        got = _one_shot(eng, modes)
        prof = eng.rhok_profile()
        r1 = _r(eng)
        rho = eng.rhok_read()
    assert r1.tobytes() == r.tobytes()
    want, flag = _initial_model(n, count)
    assert not flag
    assert got == want, [tuple(modes[m]) for m in range(count) if got[m] != want[m]]
    assert got[0] == [n << 64, 0]                               # (0, 0, 0): no padding slot was counted
    for m in range(count):
        for k in range(m + 1, count):
            if (modes[m] == -modes[k]).all():
                assert got[k] == [got[m][0], -got[m][1]]        # mode -n is the exact conjugate
    if count >= 7:
        assert got[6] == got[1] and got[1][1] != 0              # the duplicate
    assert rho.shape == (1, count) and rho.dtype == np.complex128
    assert rho[0].tobytes() == rhok_model.doubles(want).tobytes()
    assert prof["kernel_ms"] > 0.0


def test_many_tiles_per_particle_chunk():
    """n = 8200 with 4096 modes: 129 tiles in chunks of two, the last chunk with one tile of 8 live lanes.  The model is
    evaluated for every 61st mode (a mode's words do not depend on the list); the conjugates cover the rest of the
    first chunk"""
    n = 8200
    p, r, v = _params(n)
    rng = np.random.default_rng(3)
    modes = np.concatenate([np.array(SPECIAL), rng.integers(-60, 61, size=(4096 - len(SPECIAL), 3))]).astype(np.int32)
    with Engine(p) as eng:
        eng.set_state(r[0], r[1], r[2], v[0], v[1], v[2])
        got = _one_shot(eng, modes)
        r1 = _r(eng)
    pick = list(range(0, 4096, 61)) + [4095]
    want, flag = rhok_model.words(r1, p.box_length, modes[pick])
    assert not flag and [got[m] for m in pick] == want
    assert got[0] == [n << 64, 0] and got[2] == [got[1][0], -got[1][1]] and got[7] == [got[5][0], -got[5][1]]


# ---- 2. after steps ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4096, 4100])
def test_after_steps_across_re_sorts_and_in_id_order(n, monkeypatch):
    """25 steps with a re-sort every 3: the slot order is no longer the caller's.  The words equal the model's, and those
    of a second engine that is given the snapshot in id order"""
    monkeypatch.setenv("LJMD_RESORT_EVERY", "3")
    p, r, v = _params(n)
    modes = _mode_list(65)
    with Engine(p) as eng:
        eng.set_state(r[0], r[1], r[2], v[0], v[1], v[2])
        eng.compute_forces()
        eng.verlet_steps(25)
        got = _one_shot(eng, modes)
        st = eng.get_state(("r", "v"))
    r1, v1 = np.stack(st["r"]), np.stack(st["v"])
    assert r1.tobytes() != r.tobytes()
    want, flag = rhok_model.words(r1, p.box_length, modes)
    assert not flag and got == want
    with Engine(p) as other:
        other.set_state(r1[0], r1[1], r1[2], v1[0], v1[1], v1[2])
        assert _one_shot(other, modes) == got


# ---- 3. the words of a mode do not depend on the list ------------------------------------------------------------------
def test_mode_list_independence():
    n = 500
    p, r, v = _params(n)
    rng = np.random.default_rng(8)
    big = np.concatenate([_mode_list(257), rng.integers(-1023, 1024, size=(4096 - 257, 3))]).astype(np.int32)
    perm = rng.permutation(257)
    with Engine(p) as eng:
        eng.set_state(r[0], r[1], r[2], v[0], v[1], v[2])
        base = _one_shot(eng, big[:257])
        permuted = _one_shot(eng, big[:257][perm])
        alone = _one_shot(eng, big[3:4])
        full = _one_shot(eng, big)
    want, _ = _initial_model(n, 257)
    assert base == want
    assert permuted == [base[k] for k in perm]
    assert alone == [base[3]]
    assert full[:257] == base
    pick = list(range(257, 4096, 97)) + [4095]
    tail, flag = rhok_model.words(r, p.box_length, big[pick])
    assert not flag and [full[m] for m in pick] == tail


# ---- 4. positions that are not compact -------------------------------------------------------------------------------
def test_positions_spanning_several_boxes():
    n = 4096
    p, r, v = _params(n)
    L = p.box_length
    r = r.copy()
    r[0, ::5] += 3 * L
    r[1, 1::7] -= 3 * L
    r[2, 2::11] += 3 * L
    modes = _mode_list(65)
    with Engine(p) as eng:
        eng.set_state(r[0], r[1], r[2], v[0], v[1], v[2])
        got = _one_shot(eng, modes)
        r1 = _r(eng)
    assert np.ptp(r1[0]) > 2.4 * L
    want, flag = rhok_model.words(r1, L, modes)
    assert not flag and got == want


# ---- 5. range ----------------------------------------------------------------------------------------------------------
def _raw_words(eng, count):
    """ljmd_rhok_read_exact called directly: (return code, [[Re, Im] per mode] of snapshot 0) -- the words are copied even
    when the sticky word makes the call fail"""
    words = np.zeros((1, count, 2, 3), dtype=np.int64)
    rc_ = _lib.load().ljmd_rhok_read_exact(eng._h, words.ctypes.data_as(_lib.c_int64_p), None)
    u = words.view(np.uint64)
    return rc_, [[(int(words[0, m, c, 2]) << 128) + (int(u[0, m, c, 1]) << 64) + int(u[0, m, c, 0]) for c in range(2)]
                 for m in range(count)]


def test_a_nan_coordinate_sets_the_sticky_word():
    """a NaN coordinate on one live particle, written as the wrapped position of a state that is otherwise sound: the
    accumulate succeeds, both reads return LJMD_ERR_RANGE until reset, every other particle's terms are in the sums and
    the handle is not poisoned.  Without the NaN particle no flag is set: the padding slots, NaN by construction, are
    told from particles by the permutation"""
    n = 500
    p, r, v = _params(n)
    modes = _mode_list(65)
    with Engine(p) as eng:
        eng.set_state(r[0], r[1], r[2], v[0], v[1], v[2])
        eng.compute_forces()
        eng.rhok_configure(modes, 4)
        eng.rhok_accumulate()
        assert eng.rhok_read_exact().shape == (1, 65, 2)         # no flag: 12 padding slots hold NaN
        eng.rhok_reset()
        st = eng.get_state()
        bad = [a.copy() for a in st["r"]]
        bad[1][7] = np.nan
        eng.set_state(bad[0], bad[1], bad[2], v[0], v[1], v[2])
        eng.rhok_accumulate()
        assert np.isnan(_r(eng)[1, 7])
        for read in (eng.rhok_read, eng.rhok_read_exact):
            with pytest.raises(LjmdError) as ei:
                read()
            assert ei.value.code == _lib.LJMD_ERR_RANGE and "ljmd_rhok_reset" in ei.value.message
        rc_, got = _raw_words(eng, 65)
        want, flag = rhok_model.words(np.stack(bad), p.box_length, modes)
        assert rc_ == _lib.LJMD_ERR_RANGE and flag and got == want and got[0] == [(n - 1) << 64, 0]
        eng.rhok_reset()
        assert eng.rhok_read_exact().shape == (0, 65, 2) and eng.rhok_read().shape == (0, 65)
        eng.set_state(r[0], r[1], r[2], v[0], v[1], v[2])       # not poisoned
        eng.compute_forces()
        eng.verlet_steps(2)
        eng.rhok_accumulate()
        assert eng.rhok_read_exact().shape == (1, 65, 2)


# ---- 6. precision mode -------------------------------------------------------------------------------------------------
def test_words_do_not_depend_on_the_precision_mode():
    n = 16384
    p, r, v = _params(n)
    modes = _mode_list(65)
    got = {}
    for mode, code in PRECISIONS.items():
        with Engine(p, precision_mode=code) as eng:
            eng.set_state(r[0], r[1], r[2], v[0], v[1], v[2])
            eng.compute_forces()
            got[mode] = _one_shot(eng, modes)
    assert got["fp64"] == got["mixed"] == got["reproducible"]
    want, flag = rhok_model.words(r, p.box_length, modes)
    assert not flag and got["fp64"] == want


# ---- 7. the engine and the other observables are left alone ----------------------------------------------------------
def _same(a, b):
    """nested tuples / lists / dicts of arrays and scalars: bytes-equal"""
    if isinstance(a, dict):
        assert sorted(a) == sorted(b)
        for k in a:
            _same(a[k], b[k])
    elif isinstance(a, (tuple, list)):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            _same(x, y)
    elif isinstance(a, np.ndarray) and a.dtype != object:
        assert a.shape == b.shape and a.tobytes() == b.tobytes()
    elif isinstance(a, np.ndarray):
        assert a.shape == b.shape and a.tolist() == b.tolist()
    else:
        assert a == b


@pytest.mark.parametrize("mode, n", [("fp64", 4096), ("reproducible", 4096), ("mixed", 16384)])
def test_accumulates_leave_everything_else_bitwise_alone(mode, n, monkeypatch):
    """two engines run the same enqueued segments with the other five observables accumulated between them, one of them
    with density-mode accumulates enqueued back to back in between as well, across re-sorts: r, ru, v, a, the step
    records and the other five observables' results are bitwise equal"""
    monkeypatch.setenv("LJMD_RESORT_EVERY", "3")
    seg, nseg = 5, 3
    p, r, v = _params(n)
    modes = _mode_list(65)
    out = []
    for with_rhok in (False, True):
        with Engine(p, precision_mode=PRECISIONS[mode]) as eng:
            eng.set_state(r[0], r[1], r[2], v[0], v[1], v[2])
            eng.compute_forces()
            eng.rdf_configure(50)
            eng.tcf_configure(4)
            eng.stress_configure(nseg + 1)
            eng.heatflux_configure(nseg + 1)
            eng.vanhove_configure(4, 1, 32)
            if with_rhok:
                eng.rhok_configure(modes, 2 * nseg + 1)
                eng.rhok_accumulate()
            for _ in range(nseg):
                eng.enqueue_steps(seg)
                if with_rhok:
                    eng.rhok_accumulate()
                eng.rdf_accumulate()
                eng.tcf_accumulate()
                eng.stress_accumulate()
                eng.heatflux_accumulate()
                eng.vanhove_accumulate()
                if with_rhok:
                    eng.rhok_accumulate()
            scalars = np.stack(eng.collect_steps(seg * nseg))
            state = eng.get_state()
            others = (eng.rdf_read(), eng.tcf_read_exact(), eng.stress_read_exact(raw=True), eng.heatflux_read_exact(raw=True),
                      eng.vanhove_read_exact())
            words = eng.rhok_read_exact() if with_rhok else None
        out.append((scalars, state, others, words))
    (sc0, st0, ot0, _), (sc1, st1, ot1, words) = out
    assert sc0.tobytes() == sc1.tobytes()
    for key in ("r", "ru", "v", "a"):
        for a, b in zip(st0[key], st1[key]):
            assert a.tobytes() == b.tobytes(), key
    _same(ot0, ot1)
    assert words.shape == (2 * nseg + 1, 65, 2)
    for k in range(nseg):                                       # around the other accumulates: the same state twice
        assert words[1 + 2 * k].tolist() == words[2 + 2 * k].tolist()
    assert words[0].tolist() != words[1].tolist() != words[3].tolist()
    want, flag = rhok_model.words(np.stack(st1["r"]), p.box_length, modes)
    assert not flag and words[-1].tolist() == want


# ---- 8. sequence and guards ------------------------------------------------------------------------------------------
def _code(call):
    with pytest.raises(LjmdError) as ei:
        call()
    return ei.value.code, ei.value.message


def test_sequence_and_guards():
    n = 500
    p, r, v = _params(n)
    lib = _lib.load()
    modes = _mode_list(65)
    with Engine(p) as eng:
        for call in (lambda: lib.ljmd_rhok_accumulate(eng._h), lambda: lib.ljmd_rhok_read(eng._h, None, None),
                     lambda: lib.ljmd_rhok_read_exact(eng._h, None, None), lambda: lib.ljmd_rhok_reset(eng._h),
                     lambda: lib.ljmd_rhok_profile_read(eng._h, None)):
            assert call() == _lib.LJMD_ERR_STATE                                     # before configure
            assert "the density modes are not configured" in _lib.last_error(eng._h)
        eng.rhok_configure(modes, 2)                                                 # without a state
        code, msg = _code(eng.rhok_accumulate)
        assert code == _lib.LJMD_ERR_STATE and "no state" in msg
        eng.set_state(r[0], r[1], r[2], v[0], v[1], v[2])
        eng.rhok_accumulate()                                                        # a state, no accelerations: enough
        want, _ = _initial_model(n, 65)
        assert eng.rhok_read_exact()[0].tolist() == want
        eng.rhok_reset()
        eng.compute_forces()
        for bad in (-1, _lib.RHOK_MAX_SNAPSHOTS + 1):
            code, msg = _code(lambda: eng.rhok_configure(modes, bad))
            assert code == _lib.LJMD_ERR_INVALID_ARG and msg.startswith("ljmd_rhok_configure: max_snapshots"), msg
        over = modes.copy()
        over[9, 2] = _lib.RHOK_MAX_INDEX + 1
        code, msg = _code(lambda: eng.rhok_configure(over, 2))
        assert code == _lib.LJMD_ERR_INVALID_ARG and "mode 9" in msg and "1024" in msg
        code, msg = _code(lambda: eng.rhok_configure(np.zeros((_lib.RHOK_MAX_MODES + 1, 3), dtype=np.int32), 2))
        assert code == _lib.LJMD_ERR_INVALID_ARG and "n_modes = 4097" in msg
        code, msg = _code(lambda: eng.rhok_configure(np.zeros((0, 3), dtype=np.int32), 2))
        assert code == _lib.LJMD_ERR_INVALID_ARG and "n_modes = 0" in msg
        code, msg = _code(lambda: eng.rhok_configure(np.zeros((4096, 3), dtype=np.int32), 4097))
        assert code == _lib.LJMD_ERR_INVALID_ARG and "max_snapshots * n_modes" in msg
        with pytest.raises(TypeError):
            eng.rhok_configure(modes, 2.0)
        with pytest.raises(TypeError):
            eng.rhok_configure(modes.astype(np.float64), 2)
        with pytest.raises(ValueError):
            eng.rhok_configure(modes[:, :2], 2)
        assert eng.rhok_read_exact().shape == (0, 65, 2)                             # the refused calls changed nothing
        assert eng.rhok_profile()["kernel_ms"] > 0.0                                 # the accumulate before the reset

        eng.step_begin()                                                             # inside a split-phase step
        code, msg = _code(eng.rhok_accumulate)
        assert code == _lib.LJMD_ERR_STATE and "split-phase" in msg
        eng.step_finish()
        assert eng.rhok_read_exact().shape == (0, 65, 2)
        eng.set_state(r[0], r[1], r[2], v[0], v[1], v[2])
        eng.compute_forces()

        eng.rhok_accumulate()
        assert eng.rhok_read_exact()[0].tolist() == want
        eng.set_state(r[0], r[1], r[2], v[0], v[1], v[2])                            # the setters keep the series
        eng.set_accel(*eng.get_state(("a",))["a"])
        eng.set_tail_corrections(False)
        eng.rdf_configure(20)
        eng.rdf_accumulate()
        eng.tcf_configure(4)
        eng.tcf_accumulate()
        eng.stress_configure(3)
        eng.stress_accumulate()
        eng.heatflux_configure(3)
        eng.heatflux_accumulate()
        eng.vanhove_configure(4, 1, 32)
        eng.vanhove_accumulate()
        eng.migrate()                                                                # a no-op on one rank
        eng.rhok_accumulate()
        twice = eng.rhok_read_exact()
        assert twice.shape == (2, 65, 2) and twice[0].tolist() == want and twice[1].tolist() == want
        assert lib.ljmd_rhok_read(eng._h, None, None) == _lib.LJMD_OK                # every pointer may be NULL
        assert lib.ljmd_rhok_read_exact(eng._h, None, None) == _lib.LJMD_OK
        assert lib.ljmd_rhok_profile_read(eng._h, None) == _lib.LJMD_OK
        code, msg = _code(eng.rhok_accumulate)                                       # full
        assert code == _lib.LJMD_ERR_STATE and "series is full (2 snapshots" in msg
        assert eng.rhok_read_exact().tolist() == twice.tolist()
        eng.rhok_reset()
        assert eng.rhok_read().shape == (0, 65)
        eng.rhok_accumulate()
        assert eng.rhok_read_exact()[0].tolist() == want
        assert eng.stress_read_exact().shape == (1, 12) and eng.rdf_read()[1] == 1   # the others kept theirs
        assert eng.heatflux_read_exact().shape == (1, 9)

        eng.rhok_configure(modes[:3], 3)                                             # reconfigure: empty, another list
        assert eng.rhok_read_exact().shape == (0, 3, 2)
        eng.rhok_configure(modes, 0)                                                 # off
        assert lib.ljmd_rhok_read(eng._h, None, None) == _lib.LJMD_ERR_STATE
        assert lib.ljmd_rhok_accumulate(eng._h) == _lib.LJMD_ERR_STATE
        eng.rhok_configure(modes, 5)                                                 # destroyed while configured
        eng.rhok_accumulate()


def test_rank_engines_and_multi_device_handles_are_refused():
    n = 2048
    p, _r, _v = _params(n)
    lib = _lib.load()
    modes = _mode_list(5)
    for kwargs, extra in (({"rank": 1, "n_ranks": 2}, ""), ({"devices": [0, 0]}, " (multi-device handle)")):
        with Engine(p, **kwargs) as eng:
            code, msg = _code(lambda: eng.rhok_configure(modes, 4))
            assert code == _lib.LJMD_ERR_INVALID_ARG, msg
            assert msg.startswith("ljmd_rhok_configure: n_ranks = 2" + extra + ":") and "one-rank engine" in msg, msg
            assert "holds only its own particles" in msg
            eng.rhok_configure(modes, 0)                                             # off is no request
            for call in (lambda: lib.ljmd_rhok_accumulate(eng._h), lambda: lib.ljmd_rhok_read(eng._h, None, None),
                         lambda: lib.ljmd_rhok_read_exact(eng._h, None, None), lambda: lib.ljmd_rhok_reset(eng._h),
                         lambda: lib.ljmd_rhok_profile_read(eng._h, None)):
                assert call() == _lib.LJMD_ERR_STATE and "not configured" in _lib.last_error(eng._h)


# ---- 9. physics --------------------------------------------------------------------------------------------------------
def test_structure_factor_of_a_jittered_lattice():
    """n = 4096 = 16^3 particles on a simple cubic lattice, each displaced by up to 5 % of the spacing: S at the Bragg
    vector (16, 0, 0) is of order N -- the Debye-Waller factor of that jitter is about 0.92 -- and S at (1, 0, 0), where
    the lattice sum vanishes, is of order 1 at most"""
    n, cells = 4096, 16
    p, _r, v = _params(n)
    L = p.box_length
    rng = np.random.default_rng(2)
    site = np.stack([g.ravel() for g in np.meshgrid(*[np.arange(cells)] * 3, indexing="ij")]).astype(np.float64)
    r = (site + 0.5 + rng.uniform(-0.05, 0.05, size=site.shape)) * (L / cells)
    modes = np.array([(16, 0, 0), (0, 16, 0), (0, 0, 16), (1, 0, 0), (0, 1, 0), (0, 0, 1)], dtype=np.int32)
    with Engine(p) as eng:
        eng.set_state(r[0], r[1], r[2], v[0], v[1], v[2])
        eng.rhok_configure(modes, 1)
        eng.rhok_accumulate()
        rho = eng.rhok_read()
        exact = eng.rhok_read_exact()
    want, flag = rhok_model.words(r, L, modes)
    assert not flag and exact[0].tolist() == want
    k, S, err, count = analysis.static_structure_factor(rho, n, modes, L)
    assert list(count) == [3, 3] and np.isnan(err).all()
    np.testing.assert_allclose(k, [2 * np.pi / L, 2 * np.pi * 16 / L], rtol=1e-15)
    assert 0.8 * n < S[1] < n and S[0] < 2.0, S
