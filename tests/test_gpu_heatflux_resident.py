"""-m gpu: the heat flux of the resident system recorded on the one-rank engine (ljmd_heatflux_*, Engine.heatflux_*).
A snapshot is 9 exact integers: every comparison of words is equality with tests/heatflux_model.py (numpy arithmetic,
Python ints) on the state get_state returns."""
import functools
from fractions import Fraction

import numpy as np
import pytest

import heatflux_model
import stress_model
from ljmd_amd import Engine, _lib, md_types, synthetic
from ljmd_amd._lib import LjmdError

pytestmark = pytest.mark.gpu

REPRO = _lib.PRECISION_FP64_REPRODUCIBLE
MODES = {"fp64": _lib.PRECISION_FP64, "mixed": _lib.PRECISION_FP32_FORCE, "reproducible": REPRO}


def _start(eng, r, v):
    eng.set_state(r[0], r[1], r[2], v[0], v[1], v[2])
    eng.compute_forces()


def _state(eng):
    st = eng.get_state(("r", "v"))
    return np.stack(st["r"]), np.stack(st["v"])


def _one_shot(eng, max_snapshots=1):
    """configure, one accumulate -> the 9 integers"""
    eng.heatflux_configure(max_snapshots)
    eng.heatflux_accumulate()
    words = eng.heatflux_read_exact()
    assert words.shape == (1, 9)
    return list(words[0])


def _params(n, rc=None, seed=None, rho=0.8):
    """the synthetic configuration of n particles at rho = 0.8, with rc = 0.49 L or the given cutoff"""
    p, r, v = synthetic.make_config(n, seed=1000 + n if seed is None else seed, rho=rho)
    if rc is not None:
        p = md_types.init_params(n, p.box_length, p.dt, rc)
    return p, r, v


@functools.lru_cache(maxsize=None)
def _initial_model(n, rc):
    """model words of the initial configuration (the engine wraps nothing there: get_state returns the input)"""
    p, r, v = _params(n, rc)
    return heatflux_model.words(r, v, p.box_length, p.rc)


# ---- 1. one-shot words -----------------------------------------------------------------------------------------------
# n = 108, 500: the gather engine, the last live tile has 44 and 52 particles.  n = 4096: 64 full tiles, an even tile count
# and its tie rule; n = 4100: 4 live lanes in the 65th tile.  rc = 0.49 L reaches nearly half of all pairs; rc = 2.5 lets
# the walk skip tile pairs.
@pytest.mark.parametrize("n, rc", [(108, None), (500, None), (4096, None), (4100, None), (4096, 2.5), (4100, 2.5)])
def test_one_shot_words_equal_the_model(n, rc):
    p, r, v = _params(n, rc)
    with Engine(p) as eng:
        _start(eng, r, v)
        got = _one_shot(eng)
        prof = eng.heatflux_profile()
        r1, v1 = _state(eng)
        j, parts = eng.heatflux_read()
    assert r1.tobytes() == r.tobytes() and v1.tobytes() == v.tobytes()
    want, flag = _initial_model(n, rc)
    assert not flag
    assert got == want, [heatflux_model.ROWS[c] for c in range(9) if got[c] != want[c]]
    wj, wparts = heatflux_model.doubles(want, p.box_length)
    assert j.shape == (1, 3) and parts.shape == (1, 3, 3)
    assert j[0].tobytes() == wj.tobytes() and parts[0].tobytes() == wparts.tobytes()
    assert 0 < prof["tile_pairs_visited"] <= prof["tile_pairs_total"] and prof["kernel_ms"] > 0.0
    if rc is not None:
        assert prof["tile_pairs_visited"] < prof["tile_pairs_total"], prof
    assert all(x != 0 for x in got)


# ---- 2. after steps ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4096, 4100])
def test_after_steps_across_re_sorts_and_in_id_order(n, monkeypatch):
    """25 steps with a re-sort every 3: the slot order is no longer the caller's, for the positions and the velocities
    alike.  The words equal the model's, and those of a second engine that is given the snapshot in id order"""
    monkeypatch.setenv("LJMD_RESORT_EVERY", "3")
    p, r, v = _params(n, 2.5)
    with Engine(p) as eng:
        _start(eng, r, v)
        eng.verlet_steps(25)
        got = _one_shot(eng)
        prof = eng.heatflux_profile()
        r1, v1 = _state(eng)
    want, flag = heatflux_model.words(r1, v1, p.box_length, p.rc)
    assert not flag and got == want
    assert prof["tile_pairs_visited"] < prof["tile_pairs_total"]
    with Engine(p) as other:
        _start(other, r1, v1)
        assert _one_shot(other) == got


# ---- 3. positions that are not compact -------------------------------------------------------------------------------
def test_positions_spanning_several_boxes():
    """raw set_state input with particles shifted by +-3 L: the handle does not know the positions to be compact, nothing
    is skipped, and the words are those of the positions as given"""
    n = 4096
    p, r, v = _params(n, 2.5)
    L = p.box_length
    r = r.copy()
    r[0, ::5] += 3 * L
    r[1, 1::7] -= 3 * L
    r[2, 2::11] += 3 * L
    with Engine(p) as eng:
        _start(eng, r, v)
        got = _one_shot(eng)
        prof = eng.heatflux_profile()
        r1, v1 = _state(eng)
    assert np.ptp(r1[0]) > 2.4 * L
    want, flag = heatflux_model.words(r1, v1, L, p.rc)
    assert not flag and got == want
    assert prof["tile_pairs_visited"] == prof["tile_pairs_total"] > 0


# ---- 4. uniform drift --------------------------------------------------------------------------------------------------
def test_uniform_drift_ties_the_words_to_other_sums():
    """every velocity = v0: w = 2 v0 for every pair, so the new integers are tied to sums another code path produces:
      R(P[a])       ~ v0_a 2 sum_ordered (u6 - u3)        (the model's own sum of phi)
      6 R(C[a])     ~ 12 sum_b v0_b R(S_ab)               (S from ljmd_stress_read_exact on the same handle)
      0.5 R(E[a])   ~ v0_a n |v0|^2 / 2
    Bounds, from the model: the number of terms times 2^-65 (the rounding of Q) plus sum |term| 2^-52, where for C the
    'term' is (|fx wx| + |fy wy| + |fz wz|) |d_a|, which bounds every intermediate of g d_a.  The comparisons are made in
    exact rational arithmetic on the integers, so no rounding of the test's own enters.  v0 is dyadic with few bits: k2
    and k2 v_a are then exact and the E relation holds to the rounding of Q alone.  The P bound is a worst case (one
    product rounding of 2^-53 per term, one of the reference sum).  For C the worst case over all roundings of both code
    paths would be about 11 x 2^-53 sum |term|; the bound used is the stated 2^-52, which the signs of about 1e5
    independent roundings leave a wide margin to."""
    n = 500
    p, r, _v = _params(n)
    L = p.box_length
    v0 = np.array([0.75, -0.5625, 0.3125])
    v = np.repeat(v0[:, None], n, axis=1)
    with Engine(p) as eng:
        _start(eng, r, v)
        got = _one_shot(eng)
        eng.stress_configure(1)
        eng.stress_accumulate()
        S = list(eng.stress_read_exact()[0])[6:]
        r1, v1 = _state(eng)
    want, flag = heatflux_model.words(r1, v1, L, p.rc)
    assert not flag and got == want
    _s, _f, stats = heatflux_model.pair_words(r1, v1, L, p.rc)
    E, P, Cc = got[:3], got[3:6], got[6:]
    two64 = 1 << 64
    f0 = [Fraction(float(x)) for x in v0]
    Sab = [[S[0], S[3], S[4]], [S[3], S[1], S[5]], [S[4], S[5], S[2]]]
    k2 = sum(x * x for x in f0)
    for a in range(3):
        # potential
        ref = f0[a] * 2 * Fraction(stats["phi"])
        bound = Fraction(stats["pairs"]) / 2 ** 65 + Fraction(stats["abs_P"][a]) / 2 ** 52
        diff = abs(Fraction(P[a], two64) - ref)
        print("P[%d]: |diff| = %.3e, bound %.3e, value %.6e" % (a, float(diff), float(bound), float(ref)))
        assert diff <= bound and ref != 0
        # collisional: 6 C[a] against 12 sum_b v0_b S_ab; the stress side has its own Q roundings, 2 |v0_b| each
        ref = 12 * sum(f0[b] * Fraction(Sab[a][b], two64) for b in range(3))
        terms = stats["pairs"] * (1 + 2 * sum(abs(x) for x in f0))
        bound = 6 * (Fraction(terms) / 2 ** 65 + Fraction(stats["abs_C"][a]) / 2 ** 52)
        diff = abs(6 * Fraction(Cc[a], two64) - ref)
        print("C[%d]: |diff| = %.3e, bound %.3e, value %.6e" % (a, float(diff), float(bound), float(ref)))
        assert diff <= bound and ref != 0
        # convective
        ref = f0[a] * n * k2 / 2
        bound = Fraction(n) / 2 ** 65 + abs(2 * ref) / 2 ** 52
        diff = abs(Fraction(E[a], two64) / 2 - ref)
        print("E[%d]: |diff| = %.3e, bound %.3e, value %.6e" % (a, float(diff), float(bound), float(ref)))
        assert diff <= bound


# ---- 5. range ----------------------------------------------------------------------------------------------------------
def _raw_words(eng):
    """ljmd_heatflux_read_exact called directly: (return code, the 9 integers of snapshot 0) -- the words are copied even
    when the sticky word makes the call fail"""
    words = np.zeros((1, 9, 3), dtype=np.int64)
    rc_ = _lib.load().ljmd_heatflux_read_exact(eng._h, words.ctypes.data_as(_lib.c_int64_p), None)
    u = words.view(np.uint64)
    return rc_, [(int(words[0, c, 2]) << 128) + (int(u[0, c, 1]) << 64) + int(u[0, c, 0]) for c in range(9)]


def test_a_pair_out_of_range_sets_the_sticky_word():
    """two particles 1e-4 sigma apart: u6 = 1e48 is beyond 2^40.  The fp64 engine computes its forces, accumulate
    succeeds, both reads return LJMD_ERR_RANGE until reset, every other pair's terms are in the sums, the handle is not
    poisoned and steps exactly as a handle without the heat flux does"""
    n = 500
    p, r, v = _params(n)
    r = r.copy()
    r[:, 1] = r[:, 0] + np.array([1e-4, 0.0, 0.0])
    scalars = []
    for with_heatflux in (True, False):
        with Engine(p) as eng:
            _start(eng, r, v)
            if with_heatflux:
                eng.heatflux_configure(4)
                eng.heatflux_accumulate()
                for read in (eng.heatflux_read, eng.heatflux_read_exact):
                    with pytest.raises(LjmdError) as ei:
                        read()
                    assert ei.value.code == _lib.LJMD_ERR_RANGE and "ljmd_heatflux_reset" in ei.value.message
                with pytest.raises(LjmdError) as ei:            # sticky: a read clears nothing
                    eng.heatflux_read_exact()
                assert ei.value.code == _lib.LJMD_ERR_RANGE
                rc_, got = _raw_words(eng)
                r1, v1 = _state(eng)
                want, flag = heatflux_model.words(r1, v1, p.box_length, p.rc)
                assert rc_ == _lib.LJMD_ERR_RANGE and flag and got == want
                eng.heatflux_reset()
                assert eng.heatflux_read_exact().shape == (0, 9)
                j, parts = eng.heatflux_read()
                assert j.shape == (0, 3) and parts.shape == (0, 3, 3)
            scalars.append(np.stack(eng.verlet_steps(2)))      # not poisoned
    assert scalars[0].shape == (4, 2) and scalars[0].tobytes() == scalars[1].tobytes()


def test_a_velocity_out_of_range_flags_the_convective_part():
    """one velocity component of 2^15: k2 = 2^30 and k2 v = 2^45 are beyond 2^40 only in the second step, the pressure
    tensor's products (2^30) are in range: the heat flux flags, the pressure tensor of the same handle does not"""
    n = 500
    p, r, v = _params(n)
    v = v.copy()
    v[:, 7] = [2.0 ** 15, 0.0, 0.0]
    with Engine(p) as eng:
        _start(eng, r, v)
        eng.heatflux_configure(2)
        eng.stress_configure(2)
        eng.heatflux_accumulate()
        eng.stress_accumulate()
        with pytest.raises(LjmdError) as ei:
            eng.heatflux_read()
        assert ei.value.code == _lib.LJMD_ERR_RANGE and "particle's" in ei.value.message
        rc_, got = _raw_words(eng)
        sw = list(eng.stress_read_exact()[0])                   # unaffected
        r1, v1 = _state(eng)
        eng.heatflux_reset()
        assert eng.heatflux_read_exact().shape == (0, 9)
    E, kflag = heatflux_model.kinetic_words(v1)
    assert kflag and got[:3] == E
    # the pairs of particle 7 have w = 2^15 + O(1): in range, they are in the sums
    want, flag = heatflux_model.words(r1, v1, p.box_length, p.rc)
    assert flag and got == want
    swant, sflag = stress_model.words(r1, v1, p.box_length, p.rc)
    assert not sflag and sw == swant


# ---- 6. the engine and the other observables are left alone ----------------------------------------------------------
@pytest.mark.parametrize("mode, n", [("fp64", 4096), ("reproducible", 4096), ("mixed", 16384)])
def test_accumulates_leave_everything_else_bitwise_alone(mode, n, monkeypatch):
    """two engines run the same enqueued segments with g(r), MSD / VACF and the pressure tensor accumulated between them,
    one of them with heat flux accumulates enqueued back to back in between as well, across re-sorts: r, ru, v, a, the
    step records and the three other observables' results are bitwise equal"""
    monkeypatch.setenv("LJMD_RESORT_EVERY", "3")
    seg, nseg = 5, 3
    p, r, v = _params(n, 2.5)
    out = []
    for with_heatflux in (False, True):
        with Engine(p, precision_mode=MODES[mode]) as eng:
            _start(eng, r, v)
            eng.rdf_configure(50)
            eng.tcf_configure(4)
            eng.stress_configure(nseg + 1)
            if with_heatflux:
                eng.heatflux_configure(2 * nseg + 1)
                eng.heatflux_accumulate()
            for _ in range(nseg):
                eng.enqueue_steps(seg)
                if with_heatflux:
                    eng.heatflux_accumulate()
                eng.rdf_accumulate()
                eng.tcf_accumulate()
                eng.stress_accumulate()
                if with_heatflux:
                    eng.heatflux_accumulate()
            scalars = np.stack(eng.collect_steps(seg * nseg))
            state = eng.get_state()
            others = (eng.rdf_read(), eng.tcf_read_exact(), eng.stress_read_exact(raw=True))
            words = eng.heatflux_read_exact() if with_heatflux else None
        out.append((scalars, state, others, words))
    (sc0, st0, ot0, _), (sc1, st1, ot1, words) = out
    assert sc0.tobytes() == sc1.tobytes()
    for key in ("r", "ru", "v", "a"):
        for a, b in zip(st0[key], st1[key]):
            assert a.tobytes() == b.tobytes(), key
    _same(ot0, ot1)
    assert words.shape == (2 * nseg + 1, 9)
    for k in range(nseg):                                       # around the other accumulates: the same state twice
        assert list(words[1 + 2 * k]) == list(words[2 + 2 * k])
    assert list(words[0]) != list(words[1]) != list(words[3])
    if n == 4096:
        want, flag = heatflux_model.words(np.stack(st1["r"]), np.stack(st1["v"]), p.box_length, p.rc)
        assert not flag and list(words[-1]) == want


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


# ---- 7. precision mode -------------------------------------------------------------------------------------------------
def test_words_do_not_depend_on_the_precision_mode():
    """one state (n = 16 384, the smallest system of the mixed mode) on handles of the three modes: the same integers"""
    n = 16384
    p, r, v = _params(n, 2.5)
    got = {}
    for mode, code in MODES.items():
        with Engine(p, precision_mode=code) as eng:
            _start(eng, r, v)
            got[mode] = _one_shot(eng)
    assert got["fp64"] == got["mixed"] == got["reproducible"]
    assert all(x != 0 for x in got["fp64"])


# ---- 8. sequence and guards ------------------------------------------------------------------------------------------
def _code(call):
    with pytest.raises(LjmdError) as ei:
        call()
    return ei.value.code, ei.value.message


def test_sequence_and_guards():
    n = 500
    p, r, v = _params(n)
    lib = _lib.load()
    with Engine(p) as eng:
        for call in (lambda: lib.ljmd_heatflux_accumulate(eng._h), lambda: lib.ljmd_heatflux_read(eng._h, None, None, None),
                     lambda: lib.ljmd_heatflux_read_exact(eng._h, None, None), lambda: lib.ljmd_heatflux_reset(eng._h),
                     lambda: lib.ljmd_heatflux_profile_read(eng._h, None, None, None)):
            assert call() == _lib.LJMD_ERR_STATE                                     # before configure
            assert "the heat flux is not configured" in _lib.last_error(eng._h)
        eng.heatflux_configure(2)                                                    # without a state
        code, msg = _code(eng.heatflux_accumulate)
        assert code == _lib.LJMD_ERR_STATE and "no state" in msg
        eng.set_state(r[0], r[1], r[2], v[0], v[1], v[2])
        code, msg = _code(eng.heatflux_accumulate)
        assert code == _lib.LJMD_ERR_STATE and "accelerations" in msg
        eng.compute_forces()
        for bad in (-1, _lib.HEATFLUX_MAX_SNAPSHOTS + 1):
            code, msg = _code(lambda: eng.heatflux_configure(bad))
            assert code == _lib.LJMD_ERR_INVALID_ARG and msg.startswith("ljmd_heatflux_configure: max_snapshots"), msg
        with pytest.raises(TypeError):
            eng.heatflux_configure(2.0)
        assert eng.heatflux_read_exact().shape == (0, 9)                             # the refused calls changed nothing
        assert eng.heatflux_profile() == {"tile_pairs_visited": 0, "tile_pairs_total": 0, "kernel_ms": 0.0}

        eng.step_begin()                                                             # inside a split-phase step
        code, msg = _code(eng.heatflux_accumulate)
        assert code == _lib.LJMD_ERR_STATE and "split-phase" in msg
        eng.step_finish()
        assert eng.heatflux_read_exact().shape == (0, 9)
        eng.set_state(r[0], r[1], r[2], v[0], v[1], v[2])
        eng.compute_forces()

        eng.heatflux_accumulate()
        once = eng.heatflux_read_exact()
        want, _ = _initial_model(n, None)
        assert once.shape == (1, 9) and list(once[0]) == want
        eng.set_state(r[0], r[1], r[2], v[0], v[1], v[2])                            # the setters keep the series
        eng.set_accel(*eng.get_state(("a",))["a"])
        eng.set_tail_corrections(False)
        eng.rdf_configure(20)
        eng.rdf_accumulate()
        eng.tcf_configure(4)
        eng.tcf_accumulate()
        eng.stress_configure(3)
        eng.stress_accumulate()
        eng.migrate()                                                                # a no-op on one rank
        eng.heatflux_accumulate()
        twice = eng.heatflux_read_exact()
        assert twice.shape == (2, 9) and list(twice[0]) == want and list(twice[1]) == want    # no tail in the flux
        assert lib.ljmd_heatflux_read(eng._h, None, None, None) == _lib.LJMD_OK      # every pointer may be NULL
        assert lib.ljmd_heatflux_read_exact(eng._h, None, None) == _lib.LJMD_OK
        assert lib.ljmd_heatflux_profile_read(eng._h, None, None, None) == _lib.LJMD_OK
        j = np.zeros((2, 3))
        assert lib.ljmd_heatflux_read(eng._h, j.ctypes.data_as(_lib.c_double_p), None, None) == _lib.LJMD_OK   # parts NULL
        assert j[0].tobytes() == heatflux_model.doubles(want, p.box_length)[0].tobytes()
        code, msg = _code(eng.heatflux_accumulate)                                   # full
        assert code == _lib.LJMD_ERR_STATE and "series is full (2 snapshots" in msg
        assert np.array_equal(eng.heatflux_read_exact(), twice)
        eng.heatflux_reset()
        assert eng.heatflux_read()[0].shape == (0, 3)
        eng.heatflux_accumulate()
        assert list(eng.heatflux_read_exact()[0]) == want
        assert eng.stress_read_exact().shape == (1, 12) and eng.rdf_read()[1] == 1   # the others kept theirs

        eng.heatflux_configure(3)                                                    # reconfigure: empty
        assert eng.heatflux_read_exact().shape == (0, 9)
        eng.heatflux_configure(0)                                                    # off
        assert lib.ljmd_heatflux_read(eng._h, None, None, None) == _lib.LJMD_ERR_STATE
        assert lib.ljmd_heatflux_accumulate(eng._h) == _lib.LJMD_ERR_STATE
        eng.heatflux_configure(5)                                                    # destroyed while configured
        eng.heatflux_accumulate()


def test_rank_engines_and_multi_device_handles_are_refused():
    n = 2048
    p, _r, _v = _params(n)
    lib = _lib.load()
    for kwargs, extra in (({"rank": 1, "n_ranks": 2}, ""), ({"devices": [0, 0]}, " (multi-device handle)")):
        with Engine(p, **kwargs) as eng:
            code, msg = _code(lambda: eng.heatflux_configure(4))
            assert code == _lib.LJMD_ERR_INVALID_ARG, msg
            assert msg.startswith("ljmd_heatflux_configure: n_ranks = 2" + extra + ":") and "one-rank engine" in msg, msg
            assert "velocities of both particles" in msg
            eng.heatflux_configure(0)                                                # off is no request
            for call in (lambda: lib.ljmd_heatflux_accumulate(eng._h), lambda: lib.ljmd_heatflux_read(eng._h, None, None, None),
                         lambda: lib.ljmd_heatflux_read_exact(eng._h, None, None), lambda: lib.ljmd_heatflux_reset(eng._h),
                         lambda: lib.ljmd_heatflux_profile_read(eng._h, None, None, None)):
                assert call() == _lib.LJMD_ERR_STATE and "not configured" in _lib.last_error(eng._h)
