"""-m gpu: the pressure tensor of the resident system recorded on the single / sharded engine (ljmd_stress_*,
Engine.stress_*).  A snapshot is 12 exact integers: every comparison of words is equality with tests/stress_model.py
(numpy arithmetic, Python ints) on the state get_state returns."""
import functools

import numpy as np
import pytest

import stress_model
from ljmd_amd import Engine, _lib, md_types, synthetic
from ljmd_amd._lib import LjmdError
from reproducible_model import R, tail_constants

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
    """configure, one accumulate -> the 12 integers"""
    eng.stress_configure(max_snapshots)
    eng.stress_accumulate()
    words = eng.stress_read_exact()
    assert words.shape == (1, 12)
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
    return stress_model.words(r, v, p.box_length, p.rc)


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
        prof = eng.stress_profile()
        r1, v1 = _state(eng)
        pd = eng.stress_read()
    assert r1.tobytes() == r.tobytes() and v1.tobytes() == v.tobytes()
    want, flag = _initial_model(n, rc)
    assert not flag
    assert got == want, [c for c in range(12) if got[c] != want[c]]
    assert pd.shape == (1, 6) and pd[0].tobytes() == stress_model.doubles(want, p.box_length).tobytes()
    assert 0 < prof["tile_pairs_visited"] <= prof["tile_pairs_total"] and prof["kernel_ms"] > 0.0
    if rc is not None and n >= 4096:
        assert prof["tile_pairs_visited"] < prof["tile_pairs_total"], prof
    # a jittered lattice: nearly isotropic, the off-diagonals small against the diagonal
    assert np.abs(pd[0, 3:]).max() < np.abs(pd[0, :3]).min()


@pytest.mark.parametrize("n", [4096, 4100])
def test_after_steps_across_re_sorts_and_in_id_order(n, monkeypatch):
    """25 steps with a re-sort every 3: the slot order is no longer the caller's.  The words equal the model's, and those of
    a second engine that is given the snapshot in id order"""
    monkeypatch.setenv("LJMD_RESORT_EVERY", "3")
    p, r, v = _params(n, 2.5)
    with Engine(p) as eng:
        _start(eng, r, v)
        eng.verlet_steps(25)
        got = _one_shot(eng)
        prof = eng.stress_profile()
        r1, v1 = _state(eng)
    want, flag = stress_model.words(r1, v1, p.box_length, p.rc)
    assert not flag and got == want
    assert prof["tile_pairs_visited"] < prof["tile_pairs_total"]
    with Engine(p) as other:
        _start(other, r1, v1)
        assert _one_shot(other) == got


# ---- 2. ranks --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0, 0]])
def test_multi_device_handle(devices):
    """the ranks' words added on the host equal the model's -- after 40 steps, and again after an ownership migration"""
    n = 2048
    p, r, v = _params(n)
    with Engine(p, devices=devices) as eng:
        _start(eng, r, v)
        eng.verlet_steps(40)
        got = _one_shot(eng, 4)
        prof = eng.stress_profile()
        pd = eng.stress_read()
        r1, v1 = _state(eng)
        eng.migrate()
        eng.stress_accumulate()
        both = eng.stress_read_exact()
        r2, v2 = _state(eng)
    want, flag = stress_model.words(r1, v1, p.box_length, p.rc)
    assert not flag and got == want
    assert pd[0].tobytes() == stress_model.doubles(want, p.box_length).tobytes()
    assert 0 < prof["tile_pairs_visited"] <= prof["tile_pairs_total"]
    # migration moves ownership, not particles: the same set, the same integers
    assert both.shape == (2, 12) and list(both[0]) == got
    assert r2.tobytes() == r1.tobytes() and v2.tobytes() == v1.tobytes() and list(both[1]) == got


def _hip():
    import ctypes as C
    hip = C.CDLL("libamdhip64.so.7")       # already loaded by libljmd.so: same runtime instance
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMemcpy.restype = C.c_int
    return hip


def _emulated_allgather(engines):
    """device-to-device copy of every rank's own block into every other rank's exchange buffer (tests/test_gpu_sharded.py)"""
    hip = _hip()
    for e in engines:
        e.synchronize()
    for src in engines:
        sp, _tot, off, cnt = src.exchange_buffer()
        for dst in engines:
            if dst is not src:
                assert hip.hipMemcpy(dst.exchange_buffer()[0] + 8 * off, sp + 8 * off, 8 * cnt, 3) == 0
    assert hip.hipDeviceSynchronize() == 0


def test_rank_engines_return_partials_that_add_up(monkeypatch):
    """two rank engines (ljmd_create with n_ranks = 2) on one card, the test performing the exchanges: each returns the
    sums of its own rows and own velocities, the two add up to the one-rank words; read is refused; inside a split-phase
    step accumulate is refused"""
    monkeypatch.setenv("LJMD_N3_MIN_N", "100000000")          # gather kernels: no force exchange to emulate
    n = 2048
    p, r, v = _params(n)
    engines = [Engine(p, rank=g, n_ranks=2) for g in range(2)]
    try:
        for e in engines:
            e.set_state(r[0], r[1], r[2], v[0], v[1], v[2])
            e.stress_configure(2)
        _emulated_allgather(engines)
        for e in engines:
            e.forces_partial()
        for e in engines:
            e.step_begin()
        for e in engines:
            with pytest.raises(LjmdError) as ei:
                e.stress_accumulate()
            assert ei.value.code == _lib.LJMD_ERR_STATE and "split-phase" in ei.value.message
        _emulated_allgather(engines)
        for e in engines:
            e.step_finish()
        parts = []
        for e in engines:
            e.stress_accumulate()
            w = e.stress_read_exact()
            assert w.shape == (1, 12)
            parts.append(list(w[0]))
            with pytest.raises(LjmdError) as ei:
                e.stress_read()
            assert ei.value.code == _lib.LJMD_ERR_STATE and "ljmd_stress_from_exact" in ei.value.message
        shards = [_state(e) for e in engines]
    finally:
        for e in engines:
            e.close()
    r1 = np.concatenate([s[0] for s in shards], axis=1)
    v1 = np.concatenate([s[1] for s in shards], axis=1)
    S = n // 2
    for g in range(2):
        want, flag = stress_model.words(r1, v1, p.box_length, p.rc, rows=np.arange(g * S, (g + 1) * S))
        assert not flag and parts[g] == want, g
    assert parts[0] != parts[1]
    with Engine(p) as one:
        _start(one, r1, v1)
        assert _one_shot(one) == [a + b for a, b in zip(*parts)]


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
        prof = eng.stress_profile()
        r1, v1 = _state(eng)
    assert np.ptp(r1[0]) > 2.4 * L
    want, flag = stress_model.words(r1, v1, L, p.rc)
    assert not flag and got == want
    assert prof["tile_pairs_visited"] == prof["tile_pairs_total"] > 0


# ---- 4. range --------------------------------------------------------------------------------------------------------
def test_a_pair_out_of_range_sets_the_sticky_word():
    """two particles 0.05 sigma apart: f ~ 48 / r^13 is beyond 2^40.  The fp64 engine computes its forces, accumulate
    succeeds, both reads return LJMD_ERR_RANGE until reset, the handle is not poisoned and goes on stepping"""
    n = 500
    p, r, v = _params(n)
    r = r.copy()
    r[:, 1] = r[:, 0] + np.array([0.05, 0.0, 0.0])
    _want, flag = stress_model.words(r, v, p.box_length, p.rc)
    assert flag
    with Engine(p) as eng:
        _start(eng, r, v)
        eng.stress_configure(4)
        eng.stress_accumulate()
        for read in (eng.stress_read, eng.stress_read_exact):
            with pytest.raises(LjmdError) as ei:
                read()
            assert ei.value.code == _lib.LJMD_ERR_RANGE and "ljmd_stress_reset" in ei.value.message
        with pytest.raises(LjmdError) as ei:                    # sticky: a read clears nothing
            eng.stress_read_exact()
        assert ei.value.code == _lib.LJMD_ERR_RANGE
        eng.stress_reset()
        assert eng.stress_read_exact().shape == (0, 12) and eng.stress_read().shape == (0, 6)
        sc = np.stack(eng.verlet_steps(2))                      # not poisoned
        assert sc.shape == (4, 2)


# ---- 5. the engine is left alone -------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode, n", [("fp64", 4096), ("reproducible", 4096), ("mixed", 16384)])
def test_accumulates_leave_the_trajectory_bitwise_alone(mode, n, monkeypatch):
    """two engines run the same enqueued segments, one with accumulates enqueued back to back between them, across
    re-sorts: r, ru, v, a and the step records are bitwise equal"""
    monkeypatch.setenv("LJMD_RESORT_EVERY", "3")
    seg, nseg = 5, 3
    p, r, v = _params(n, 2.5)
    out = []
    for with_stress in (False, True):
        with Engine(p, precision_mode=MODES[mode]) as eng:
            _start(eng, r, v)
            if with_stress:
                eng.stress_configure(2 * nseg + 1)
                eng.stress_accumulate()
            for _ in range(nseg):
                eng.enqueue_steps(seg)
                if with_stress:
                    eng.stress_accumulate()
                    eng.stress_accumulate()
            scalars = np.stack(eng.collect_steps(seg * nseg))
            state = eng.get_state()
            words = eng.stress_read_exact() if with_stress else None
        out.append((scalars, state, words))
    (sc0, st0, _), (sc1, st1, words) = out
    assert sc0.tobytes() == sc1.tobytes()
    for key in ("r", "ru", "v", "a"):
        for a, b in zip(st0[key], st1[key]):
            assert a.tobytes() == b.tobytes(), key
    assert words.shape == (2 * nseg + 1, 12)
    for k in range(nseg):                                       # back to back: the same state twice
        assert list(words[1 + 2 * k]) == list(words[2 + 2 * k])
    assert list(words[0]) != list(words[1]) != list(words[3])
    if n == 4096:
        want, flag = stress_model.words(np.stack(st1["r"]), np.stack(st1["v"]), p.box_length, p.rc)
        assert not flag and list(words[-1]) == want


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


# ---- 6. identities and the oracle ------------------------------------------------------------------------------------
def test_identities_in_the_reproducible_mode_without_tail():
    n = 500
    p, r, v = _params(n)
    with Engine(p, precision_mode=REPRO) as eng:
        eng.set_tail_corrections(False)
        eng.set_state(r[0], r[1], r[2], v[0], v[1], v[2])
        _e, d_epot, _dd = eng.compute_forces()
        ekin = eng.kinetic_energy()
        w = _one_shot(eng)
    K, S = w[:6], w[6:]
    assert np.float64(0.5 * ((R(K[0]) + R(K[1])) + R(K[2]))).tobytes() == np.float64(ekin).tobytes()
    _S, _flag, mdu_ordered = stress_model.virial_words(r, p.box_length, p.rc)
    # Roundings per pair between the exact 2 u^6 - u^3 and a diagonal term f_a d_a: three in each product (m d, (m d) u,
    # f d), three in r2, one in u (u r2 = 1 only to a rounding) and one in mdu: about 9 -- doubled for margin: 16.  Each is
    # 2^-53 relative, and the three diagonal terms of a pair add up to mdu u r2.  24 = 12 x the two orders of a pair.
    bound = 16 * 2.0 ** -53 * 24 * (0.5 * mdu_ordered)
    diff = abs(12.0 * ((R(S[0]) + R(S[1])) + R(S[2])) + d_epot)
    print("trace identity: |12 tr S + d_epot| = %.3e, bound %.3e, d_epot = %.6e" % (diff, bound, d_epot))
    assert diff <= bound


@pytest.mark.parametrize("n", [108, 4096])
def test_isotropic_pressure_against_the_oracle(oracle, n):
    """(p_xx + p_yy + p_zz) / 3 in fp64 mode against the pressure formed from the oracle's ekin and d_epot (tail off) for
    the same state.  Tolerance: tests/test_gpu_parity.py bounds d_epot of one force call at n <= 4096 by 1e-13 relative
    (REL_SCALAR); carried through / (3 V)"""
    p, r, v = _params(n)
    po = oracle.derive_params(p.n, p.box_length, p.dt, p.rc)
    oracle.set_tail_corrections(False)
    try:
        e_o, d_o, _dd, _ax, _ay, _az = oracle.compute_forces(po, r[0].copy(), r[1].copy(), r[2].copy())
    finally:
        oracle.set_tail_corrections(True)
    ekin_o = oracle.ekin_fused(v[0], v[1], v[2])
    _etot, _temp, press_o = oracle.observables(po, e_o, ekin_o, d_o)
    with Engine(p) as eng:
        _start(eng, r, v)
        eng.stress_configure(1)
        eng.stress_accumulate()
        pd = eng.stress_read()[0]
    V = (p.box_length * p.box_length) * p.box_length
    iso = ((pd[0] + pd[1]) + pd[2]) / 3.0
    tol = 1e-13 * abs(d_o) / (3.0 * V)
    print("n = %d: p_iso = %.15e, oracle %.15e, |diff| = %.3e, tolerance %.3e" % (n, iso, press_o, abs(iso - press_o), tol))
    assert abs(iso - press_o) <= tol
    assert tail_constants(n, p.box_length, p.rc)[1] != 0.0      # (the tail the oracle left out is not nothing)


# ---- 7. sequence and guards ------------------------------------------------------------------------------------------
def _code(call):
    with pytest.raises(LjmdError) as ei:
        call()
    return ei.value.code, ei.value.message


def test_sequence_and_guards():
    n = 500
    p, r, v = _params(n)
    lib = _lib.load()
    with Engine(p) as eng:
        for call in (lambda: lib.ljmd_stress_accumulate(eng._h), lambda: lib.ljmd_stress_read(eng._h, None, None),
                     lambda: lib.ljmd_stress_read_exact(eng._h, None, None), lambda: lib.ljmd_stress_reset(eng._h),
                     lambda: lib.ljmd_stress_profile_read(eng._h, None, None, None)):
            assert call() == _lib.LJMD_ERR_STATE                                     # before configure
            assert "not configured" in _lib.last_error(eng._h)
        eng.stress_configure(2)                                                      # without a state
        code, msg = _code(eng.stress_accumulate)
        assert code == _lib.LJMD_ERR_STATE and "no state" in msg
        eng.set_state(r[0], r[1], r[2], v[0], v[1], v[2])
        code, msg = _code(eng.stress_accumulate)
        assert code == _lib.LJMD_ERR_STATE and "accelerations" in msg
        eng.compute_forces()
        for bad in (-1, _lib.STRESS_MAX_SNAPSHOTS + 1):
            code, msg = _code(lambda: eng.stress_configure(bad))
            assert code == _lib.LJMD_ERR_INVALID_ARG and msg.startswith("ljmd_stress_configure: max_snapshots"), msg
        with pytest.raises(TypeError):
            eng.stress_configure(2.0)
        assert eng.stress_read_exact().shape == (0, 12)                              # the refused calls changed nothing
        assert eng.stress_profile() == {"tile_pairs_visited": 0, "tile_pairs_total": 0, "kernel_ms": 0.0}

        eng.stress_accumulate()
        once = eng.stress_read_exact()
        want, _ = _initial_model(n, None)
        assert once.shape == (1, 12) and list(once[0]) == want
        eng.set_state(r[0], r[1], r[2], v[0], v[1], v[2])                            # the setters keep the series
        eng.set_accel(*eng.get_state(("a",))["a"])
        eng.set_tail_corrections(False)
        eng.rdf_configure(20)
        eng.rdf_accumulate()
        eng.tcf_configure(4)
        eng.tcf_accumulate()
        eng.migrate()                                                                # a no-op on one rank
        eng.stress_accumulate()
        twice = eng.stress_read_exact()
        assert twice.shape == (2, 12) and list(twice[0]) == want and list(twice[1]) == want   # no tail in the tensor
        assert lib.ljmd_stress_read(eng._h, None, None) == _lib.LJMD_OK              # every pointer may be NULL
        assert lib.ljmd_stress_read_exact(eng._h, None, None) == _lib.LJMD_OK
        assert lib.ljmd_stress_profile_read(eng._h, None, None, None) == _lib.LJMD_OK
        code, msg = _code(eng.stress_accumulate)                                     # full
        assert code == _lib.LJMD_ERR_STATE and "series is full (2 snapshots" in msg
        assert np.array_equal(eng.stress_read_exact(), twice)
        eng.stress_reset()
        assert eng.stress_read().shape == (0, 6)
        eng.stress_accumulate()
        assert list(eng.stress_read_exact()[0]) == want

        eng.stress_configure(3)                                                      # reconfigure: empty
        assert eng.stress_read_exact().shape == (0, 12)
        eng.stress_configure(0)                                                      # off
        assert lib.ljmd_stress_read(eng._h, None, None) == _lib.LJMD_ERR_STATE
        assert lib.ljmd_stress_accumulate(eng._h) == _lib.LJMD_ERR_STATE
        eng.stress_configure(5)                                                      # destroyed while configured
        eng.stress_accumulate()
