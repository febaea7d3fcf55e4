"""-m gpu: MSD / VACF of the resident system accumulated on a one-rank engine (ljmd_tcf_*, Engine.tcf_*).  The sums are
exact integers: every comparison is equality with tests/tcf_model.py (the definition of include/ljmd.h in numpy and
Python ints) fed the ru, v that get_state returns at each snapshot; the quotients are R(S) / (n count) bit for bit.  The
one tolerance is the project's own, 1e-13 max|value| against the reference's arithmetic (analysis.compute_*_timeorig)
on the same snapshots."""
import numpy as np
import pytest

import tcf_model
from ljmd_amd import Engine, _lib, analysis, md_types, synthetic
from ljmd_amd._lib import LjmdError

pytestmark = pytest.mark.gpu

MSD, VACF = tcf_model.MSD, tcf_model.VACF


def _close(a, b):
    return a.shape == b.shape and np.max(np.abs(a - b)) <= 1e-13 * np.max(np.abs(b))


def _config(n, seed):
    """n = 2: two particles about 1.1 sigma apart in a box of 4 sigma (synthetic.make_config(2) puts them 0.68 sigma
    apart in a box of 1.36: within a few steps the velocities leave the range |term| < 2^40 of the sums)"""
    if n != 2:
        return synthetic.make_config(n, seed=seed)
    rng = np.random.Generator(np.random.PCG64(seed))
    r0 = 1.0 + rng.random(3)
    u = rng.normal(size=3)
    r = np.stack([r0, r0 + (1.05 + 0.1 * rng.random()) * u / np.linalg.norm(u)], axis=1)      # [3, 2]
    v1 = rng.normal(0.0, 0.5, size=3)
    return md_types.init_params(2, 4.0, 0.005, 1.9), r, np.stack([v1, -v1], axis=1)


def _start(eng, r, v):
    eng.set_state(r[0], r[1], r[2], v[0], v[1], v[2])
    eng.compute_forces()


def _snapshot(eng):
    st = eng.get_state(("ru", "v"))
    return np.stack(st["ru"]), np.stack(st["v"])


def _take(eng, model, keep=None):
    """one snapshot into the engine's sums and, from get_state, into the model's"""
    eng.tcf_accumulate()
    ru, v = _snapshot(eng)
    model.push(ru, v)
    if keep is not None:
        keep.append((ru, v))


def _assert_equals_model(eng, m, n):
    """tcf_read_exact == the model's integers, tcf_read == the model's quotients bitwise, the counts the model's"""
    sums, counts, snaps = eng.tcf_read_exact()
    msd, vacf, counts2, snaps2 = eng.tcf_read()
    assert not m.range_flag
    assert snaps == snaps2 and np.array_equal(counts, counts2)
    assert np.array_equal(counts, m.counts), (counts, m.counts)
    for kind, got in ((MSD, msd), (VACF, vacf)):
        assert list(sums[kind]) == m.S[kind], (kind, list(sums[kind]), m.S[kind])
        assert got.tobytes() == m.result(kind, n).tobytes(), (kind, got, m.result(kind, n))
    return sums, counts, msd, vacf


# ---- 1. sizes at the kernels' edges ----------------------------------------------------------------------------------
# thread, wave and 1024-id block boundaries; 1000 is the largest system kept in the caller's order, from 1024 on the
# engine k-d sorts at set_state
PAIRS = [(4, 1), (5, 2), (3, 5), (6, 6)]
SIZES = [2, 63, 64, 65, 255, 257, 1000, 1023, 1025, 2048, 4096]


@pytest.mark.parametrize("n, max_lag, stride", [(n, *PAIRS[k % len(PAIRS)]) for k, n in enumerate(SIZES)])
def test_sizes_at_the_kernels_edges(n, max_lag, stride):
    n_snap, apart = 10, 5
    p, r, v = _config(n, 300 + n)
    m = tcf_model.TcfModel(max_lag, stride)
    kept = []
    with Engine(p) as eng:
        _start(eng, r, v)
        eng.tcf_configure(max_lag, stride)
        _take(eng, m, kept)
        for _ in range(n_snap - 1):
            eng.verlet_steps(apart)
            _take(eng, m, kept)
        sums, counts, msd, vacf = _assert_equals_model(eng, m, n)
        assert eng.tcf_read()[3] == n_snap
        prof = eng.tcf_profile()
    assert np.array_equal(counts, tcf_model.reference_counts(n_snap, max_lag, stride))
    assert prof["kernel_ms"] > 0.0 and 0 <= prof["origins_live"] <= max_lag // stride + 1
    ru = np.stack([k[0] for k in kept])                       # [n_snap, 3, n]
    vv = np.stack([k[1] for k in kept])
    assert _close(msd, analysis.compute_msd_tau_timeorig(ru[:, 0], ru[:, 1], ru[:, 2], max_lag, stride))
    assert _close(vacf, analysis.compute_vacf_tau_timeorig(vv[:, 0], vv[:, 1], vv[:, 2], max_lag, stride))
    assert int(sums[VACF, 0]) > 0 and int(sums[MSD, 0]) == 0 and max(int(x) for x in sums[MSD]) > 0


# ---- 2. identity across re-sorts -------------------------------------------------------------------------------------
def test_identity_across_resorts(monkeypatch):
    """a re-sort every 3 steps falls between every two snapshots 5 steps apart: a term must pair a particle with
    itself, whatever slot it is in.  A slot-paired sum differs from the model and pairs particles up to a box apart."""
    monkeypatch.setenv("LJMD_RESORT_EVERY", "3")
    n, max_lag = 2048, 6
    p, r, v = synthetic.make_config(n, seed=12)
    m = tcf_model.TcfModel(max_lag, 1)
    with Engine(p) as eng:
        _start(eng, r, v)
        eng.tcf_configure(max_lag, 1)
        _take(eng, m)
        for _ in range(11):
            eng.verlet_steps(5)
            _take(eng, m)
        _, counts, msd, _ = _assert_equals_model(eng, m, n)
    assert np.array_equal(counts, tcf_model.reference_counts(12, max_lag, 1))
    assert 0.0 < msd[max_lag] < 1.0                           # (1 sigma)^2 after 30 steps of dt = 0.005


# ---- 3. no disturbance, no synchronisation ---------------------------------------------------------------------------
def test_accumulation_between_enqueued_segments():
    """segments and accumulates enqueued back to back, as md_simulation_gpu does; n = 2048 re-sorts every 200 steps, so
    the 250 steps cross a re-sort"""
    n, seg, nseg, max_lag = 2048, 50, 5, 4
    p, r, v = synthetic.make_config(n, seed=11)
    m = tcf_model.TcfModel(max_lag, 1)
    with Engine(p) as ref:                                    # stepped synchronously, without the feature
        _start(ref, r, v)
        ref_scalars = []
        for _ in range(nseg):
            ref_scalars.append(np.stack(ref.verlet_steps(seg)))
            m.push(*_snapshot(ref))
        ref_state = ref.get_state()
    with Engine(p) as eng:
        _start(eng, r, v)
        eng.tcf_configure(max_lag, 1)
        eng.rdf_configure(150, 2.5)
        for _ in range(nseg):
            eng.enqueue_steps(seg)
            eng.tcf_accumulate()
            eng.rdf_accumulate()
        scalars = np.stack(eng.collect_steps(seg * nseg))
        _assert_equals_model(eng, m, n)
        assert eng.tcf_read()[3] == nseg and eng.rdf_read()[1] == nseg
        state = eng.get_state()
    assert scalars.tobytes() == np.concatenate(ref_scalars, axis=1).tobytes()
    for key in ("r", "ru", "v", "a"):
        for got, exp in zip(state[key], ref_state[key]):
            assert got.tobytes() == exp.tobytes(), key


# ---- 4. ring wrap, many slices ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, max_lag, n_snap", [(108, 40, 100), (64, 511, 520)])
def test_ring_wrap_and_many_slices(n, max_lag, n_snap):
    """max_lag = 511 with stride 1: 512 ring slots, every one reused; 511 live origins and the lag-0 entry"""
    p, r, v = synthetic.make_config(n, seed=61)
    m = tcf_model.TcfModel(max_lag, 1)
    with Engine(p) as eng:
        _start(eng, r, v)
        eng.tcf_configure(max_lag, 1)
        for s in range(n_snap):
            if s:
                eng.verlet_steps(1)
            _take(eng, m)
        _, counts, _, _ = _assert_equals_model(eng, m, n)
        assert eng.tcf_profile()["origins_live"] == max_lag
    assert np.array_equal(counts, tcf_model.reference_counts(n_snap, max_lag, 1))


def test_slices_of_more_than_one_origin():
    """n = 33000 pads to 33 particle blocks, so the planner wants 32 slices and, from 33 live origins on, cuts them two to
    a slice (tests/tcf_host pins this): the terms kernel walks more than one origin of a slice, 33 and 35 live origins
    leave a last slice of one origin, 34, 36 and 37 full ones, and the lag-0 entry lies behind either.  Every smaller
    system of this file has slices of one origin."""
    n, max_lag, n_snap = 33000, 37, 41
    p, r, v = synthetic.make_config(n, seed=62)
    m = tcf_model.TcfModel(max_lag, 1)
    with Engine(p) as eng:
        _start(eng, r, v)
        eng.tcf_configure(max_lag, 1)
        for s in range(n_snap):
            if s:
                eng.verlet_steps(1)
            _take(eng, m)
        _, counts, _, _ = _assert_equals_model(eng, m, n)
        assert eng.tcf_profile()["origins_live"] == max_lag
    assert np.array_equal(counts, tcf_model.reference_counts(n_snap, max_lag, 1))


# ---- 5. trajectories -------------------------------------------------------------------------------------------------
def test_trajectories_reset_reconfigure_off_and_destroy():
    n, max_lag, stride = 500, 3, 1
    p, r, v = synthetic.make_config(n, seed=71)
    lib = _lib.load()
    m = tcf_model.TcfModel(max_lag, stride)
    with Engine(p) as eng:
        _start(eng, r, v)
        eng.tcf_configure(max_lag, stride)
        for s in range(3):
            if s:
                eng.verlet_steps(4)
            _take(eng, m)
        first, counts, _, _ = _assert_equals_model(eng, m, n)

        st = eng.get_state(("ru", "a"))                       # these leave everything alone
        eng.set_unwrapped(*st["ru"])
        eng.set_accel(*st["a"])
        eng.set_tail_corrections(True)
        eng.rdf_configure(20)
        eng.rdf_accumulate()
        eng.migrate()                                         # a no-op on one rank
        same, counts2, snaps = eng.tcf_read_exact()
        assert snaps == 3 and np.array_equal(same, first) and np.array_equal(counts2, counts)
        eng.verlet_steps(4)
        _take(eng, m)                                         # the origins are still there
        _assert_equals_model(eng, m, n)

        eng.set_state(r[0], r[1], r[2], v[0], v[1], v[2])     # a new trajectory: origins dropped, sums and counts kept
        before, counts, snaps = eng.tcf_read_exact()
        assert snaps == 4 and list(before[MSD]) == m.S[MSD] and np.array_equal(counts, m.counts)
        eng.compute_forces()
        m.new_trajectory()
        _take(eng, m)                                         # no origin is live: nothing added
        same, counts2, snaps = eng.tcf_read_exact()
        assert snaps == 5 and np.array_equal(same, before) and np.array_equal(counts2, counts)
        eng.verlet_steps(4)
        _take(eng, m)
        more, _, _, _ = _assert_equals_model(eng, m, n)       # both trajectories average together
        assert not np.array_equal(more, before)

        eng.tcf_reset()
        sums, counts, snaps = eng.tcf_read_exact()
        assert snaps == 0 and not counts.any() and not any(sums.ravel())
        m.reset()
        _take(eng, m)                                         # numbering restarted: snapshot 0 meets nothing
        eng.verlet_steps(2)
        _take(eng, m)
        _assert_equals_model(eng, m, n)

        eng.tcf_configure(5, 2)                               # reconfigure: new shape, zeroed
        sums, counts, snaps = eng.tcf_read_exact()
        assert snaps == 0 and sums.shape == (2, 6) and counts.shape == (6,) and not counts.any() and not any(sums.ravel())
        eng.tcf_configure(0)                                  # off
        assert lib.ljmd_tcf_read(eng._h, None, None, None, None) == _lib.LJMD_ERR_STATE
        assert lib.ljmd_tcf_accumulate(eng._h) == _lib.LJMD_ERR_STATE
        eng.verlet_steps(2)
        eng.tcf_configure(4, 1)                               # destroyed while configured, launches in flight
        eng.tcf_accumulate()
        eng.verlet_steps(1)
        eng.tcf_accumulate()


# ---- 6. range --------------------------------------------------------------------------------------------------------
def test_range_word_is_sticky_until_reset():
    n = 108
    p, r, v = synthetic.make_config(n, seed=81)
    m = tcf_model.TcfModel(4, 1)
    with Engine(p) as eng:
        _start(eng, r, v)
        eng.tcf_configure(4, 1)
        _take(eng, m)
        ru = [a.copy() for a in eng.get_state(("ru",))["ru"]]
        ru[1][5] += 2.0 ** 21                                 # d^2 = 2^42 >= 2^40
        eng.set_unwrapped(*ru)
        _take(eng, m)
        assert m.range_flag
        for read in (eng.tcf_read, eng.tcf_read_exact):
            with pytest.raises(LjmdError) as ei:
                read()
            assert ei.value.code == _lib.LJMD_ERR_RANGE and ei.value.message.startswith("ljmd_tcf_read"), ei.value.message
        eng.verlet_steps(4)                                   # the handle still steps: not poisoned
        with pytest.raises(LjmdError) as ei:                  # sticky
            eng.tcf_read()
        assert ei.value.code == _lib.LJMD_ERR_RANGE
        eng.tcf_reset()
        _start(eng, r, v)                                     # sound unwrapped coordinates again
        m = tcf_model.TcfModel(4, 1)
        _take(eng, m)
        eng.verlet_steps(2)
        _take(eng, m)
        _assert_equals_model(eng, m, n)
        assert eng.tcf_read()[3] == 2


# ---- 7. modes --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, mode, n_snap, max_lag", [(500, _lib.PRECISION_FP64_REPRODUCIBLE, 6, 3),
                                                       (16384, _lib.PRECISION_FP32_FORCE, 4, 3)])
def test_precision_modes(n, mode, n_snap, max_lag):
    p, r, v = synthetic.make_config(n, seed=41)
    m = tcf_model.TcfModel(max_lag, 1)
    with Engine(p, precision_mode=mode) as eng:
        _start(eng, r, v)
        eng.tcf_configure(max_lag, 1)
        _take(eng, m)
        for _ in range(n_snap - 1):
            eng.verlet_steps(5)
            _take(eng, m)
        _, counts, _, _ = _assert_equals_model(eng, m, n)
    assert np.array_equal(counts, tcf_model.reference_counts(n_snap, max_lag, 1))


# ---- 8. guards and sequence ------------------------------------------------------------------------------------------
def _code(call):
    with pytest.raises(LjmdError) as ei:
        call()
    return ei.value.code, ei.value.message


def test_sequence_and_guards():
    n = 500
    p, r, v = synthetic.make_config(n, seed=91)
    lib = _lib.load()
    with Engine(p) as eng:
        assert lib.ljmd_tcf_accumulate(eng._h) == _lib.LJMD_ERR_STATE                # before configure
        assert "ljmd_tcf_accumulate: MSD / VACF is not configured" in _lib.last_error()
        assert lib.ljmd_tcf_read(eng._h, None, None, None, None) == _lib.LJMD_ERR_STATE
        assert lib.ljmd_tcf_read_exact(eng._h, None, None, None) == _lib.LJMD_ERR_STATE
        assert lib.ljmd_tcf_reset(eng._h) == _lib.LJMD_ERR_STATE
        assert lib.ljmd_tcf_profile_read(eng._h, None, None) == _lib.LJMD_ERR_STATE
        assert "ljmd_tcf_profile_read: MSD / VACF is not configured" in _lib.last_error()
        eng.tcf_configure(3, 1)                                                      # without a state
        code, msg = _code(eng.tcf_accumulate)
        assert code == _lib.LJMD_ERR_STATE and "no state" in msg
        eng.set_state(r[0], r[1], r[2], v[0], v[1], v[2])
        code, msg = _code(eng.tcf_accumulate)
        assert code == _lib.LJMD_ERR_STATE and "accelerations" in msg
        eng.compute_forces()
        for bad, text in (((-1, 1), "ljmd_tcf_configure: max_lag = -1"), ((4097, 16), "ljmd_tcf_configure: max_lag = 4097"),
                          ((3, 0), "ljmd_tcf_configure: origin_stride"), ((3, -2), "ljmd_tcf_configure: origin_stride"),
                          ((512, 1), "ljmd_tcf_configure: max_lag / origin_stride + 1 = 513"),
                          ((1024, 2), "ljmd_tcf_configure: max_lag / origin_stride + 1 = 513")):
            code, msg = _code(lambda: eng.tcf_configure(*bad))
            assert code == _lib.LJMD_ERR_INVALID_ARG and msg.startswith(text), msg
        sums, counts, snaps = eng.tcf_read_exact()                                   # the refused calls changed nothing
        assert snaps == 0 and sums.shape == (2, 4) and not counts.any() and not any(sums.ravel())
        assert eng.tcf_profile() == {"kernel_ms": 0.0, "origins_live": 0}

        eng.step_begin()                                                             # inside a split-phase step
        code, msg = _code(eng.tcf_accumulate)
        assert code == _lib.LJMD_ERR_STATE and "split-phase" in msg
        eng.step_finish()
        assert eng.tcf_read_exact()[2] == 0

        m = tcf_model.TcfModel(3, 1)
        _take(eng, m)
        eng.verlet_steps(2)
        _take(eng, m)
        first, counts, _, _ = _assert_equals_model(eng, m, n)
        again, counts2, snaps = eng.tcf_read_exact()                                 # read clears nothing
        assert snaps == 2 and np.array_equal(again, first) and np.array_equal(counts2, counts)
        assert lib.ljmd_tcf_read(eng._h, None, None, None, None) == _lib.LJMD_OK     # every pointer may be NULL
        assert lib.ljmd_tcf_read_exact(eng._h, None, None, None) == _lib.LJMD_OK
        assert lib.ljmd_tcf_profile_read(eng._h, None, None) == _lib.LJMD_OK
        assert eng.tcf_profile()["origins_live"] == 1


@pytest.mark.parametrize("kw", [{"devices": [0, 0]}, {"rank": 0, "n_ranks": 2}])
def test_rank_engines_and_multi_device_handles_are_refused(kw):
    n = 1024
    p, r, v = synthetic.make_config(n, seed=95)
    lib = _lib.load()
    with Engine(p, **kw) as eng:
        eng.set_state(r[0], r[1], r[2], v[0], v[1], v[2])
        code, msg = _code(lambda: eng.tcf_configure(4, 1))
        assert code == _lib.LJMD_ERR_INVALID_ARG and msg.startswith("ljmd_tcf_configure: n_ranks = 2"), msg
        assert "one-rank engine" in msg
        for rc in (lib.ljmd_tcf_accumulate(eng._h), lib.ljmd_tcf_read(eng._h, None, None, None, None),
                   lib.ljmd_tcf_read_exact(eng._h, None, None, None), lib.ljmd_tcf_reset(eng._h),
                   lib.ljmd_tcf_profile_read(eng._h, None, None)):
            assert rc == _lib.LJMD_ERR_STATE and "not configured" in _lib.last_error()
        eng.tcf_configure(0)                                                         # off is accepted anywhere
