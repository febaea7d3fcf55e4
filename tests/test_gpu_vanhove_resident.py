"""-m gpu: the van Hove self-correlation of the resident system accumulated on a one-rank engine (ljmd_vanhove_*,
Engine.vanhove_*).  Counts and sums are exact integers: every comparison is equality with tests/vanhove_model.py (the
definition of include/ljmd.h in numpy and Python ints) fed the ru that get_state returns at each snapshot; the
quotients are R(S) / (n count) bit for bit.  No tolerance anywhere."""
import numpy as np
import pytest

import tcf_model
import vanhove_model
from ljmd_amd import Engine, _lib, synthetic
from ljmd_amd._lib import LjmdError
from test_gpu_tcf_resident import _config
from vanhove_model import S2, S4, VanHoveModel

pytestmark = pytest.mark.gpu


def _start(eng, r, v):
    eng.set_state(r[0], r[1], r[2], v[0], v[1], v[2])
    eng.compute_forces()


def _take(eng, model):
    """one snapshot into the engine's counts and sums and, from get_state, into the model's"""
    eng.vanhove_accumulate()
    model.push(np.stack(eng.get_state(("ru",))["ru"]))


def _assert_equals_model(eng, m, n, flagged=False):
    """vanhove_read_exact == the model's integers, vanhove_read == the model's quotients bitwise, every row of the
    histogram sums to n count"""
    hist, sums, counts, snaps = eng.vanhove_read_exact()
    hist2, r2, r4, counts2, snaps2 = eng.vanhove_read()
    assert m.range_flag == flagged
    assert snaps == snaps2 and np.array_equal(counts, counts2) and np.array_equal(hist, hist2)
    assert np.array_equal(counts, m.counts), (counts, m.counts)
    assert hist.dtype == np.uint64 and hist.shape == m.H.shape and np.array_equal(hist, m.H)
    assert np.array_equal(hist.sum(axis=1), np.uint64(n) * counts.astype(np.uint64))
    for kind, got in ((S2, r2), (S4, r4)):
        assert list(sums[kind]) == m.S[kind], (kind, list(sums[kind]), m.S[kind])
        assert got.tobytes() == m.result(kind, n).tobytes(), (kind, got, m.result(kind, n))
    return hist, sums, counts


# ---- 1. sizes at the kernels' edges ----------------------------------------------------------------------------------
# thread, wave and 1024-id block boundaries (the padding ids of a block must not be counted); 1000 is the largest system
# kept in the caller's order, from 1024 on the engine k-d sorts at set_state.  nbins: one bin, a wave, a wave and one, the
# limit.  A thermal particle (T = 1) moves about 0.04 sigma between two snapshots 5 steps apart.
PAIRS = [(4, 1), (5, 2), (3, 5), (6, 6)]
SIZES = [2, 63, 64, 65, 255, 257, 1000, 1023, 1025, 2048, 4096]
NBINS = [1, 64, 65, 4096]


@pytest.mark.parametrize("n, max_lag, stride, nbins",
                         [(n, *PAIRS[k % 4], NBINS[(k + k // 4) % 4]) for k, n in enumerate(SIZES)])
def test_sizes_at_the_kernels_edges(n, max_lag, stride, nbins):
    n_snap, apart = 10, 5
    rmax = 0.03 if n == 2 else 0.1
    p, r, v = _config(n, 300 + n)
    m = VanHoveModel(max_lag, stride, nbins, rmax)
    with Engine(p) as eng:
        _start(eng, r, v)
        eng.vanhove_configure(max_lag, stride, nbins, rmax)
        _take(eng, m)
        for _ in range(n_snap - 1):
            eng.verlet_steps(apart)
            _take(eng, m)
        hist, sums, counts = _assert_equals_model(eng, m, n)
        assert eng.vanhove_read()[4] == n_snap
        prof = eng.vanhove_profile()
    assert np.array_equal(counts, tcf_model.reference_counts(n_snap, max_lag, stride))
    assert prof["kernel_ms"] > 0.0 and 0 <= prof["origins_live"] <= max_lag // stride + 1
    # from the model: the longest lag that was met overflows for some particles, and bin 0 is not the only bin hit
    longest = max(l for l in range(max_lag + 1) if m.counts[l])
    assert m.H[longest, nbins] > 0 and np.count_nonzero(m.H.sum(axis=0)) >= 2
    assert nbins == 1 or m.H[:, 1:nbins].sum() > 0
    assert m.H[0, 0] == n * m.counts[0] and m.S[S2][0] == 0 and m.S[S4][0] == 0      # lag 0: no displacement
    assert max(m.S[S2]) > 0 and max(m.S[S4]) > 0


# ---- 2. origins per slice --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [255, 1025])
@pytest.mark.parametrize("chunk", [1, 2, 5, 64])
def test_results_do_not_depend_on_the_slices(n, chunk, monkeypatch):
    """LJMD_VANHOVE_CHUNK origins per slice: one, two, an odd number that leaves a shorter last slice, and more than are
    live (one slice, a workgroup walks all 8 origins and the lag-0 row)"""
    monkeypatch.setenv("LJMD_VANHOVE_CHUNK", str(chunk))
    max_lag, n_snap = 8, 12
    p, r, v = synthetic.make_config(n, seed=500 + n)
    m = VanHoveModel(max_lag, 1, 96, 0.2)
    with Engine(p) as eng:
        _start(eng, r, v)
        eng.vanhove_configure(max_lag, 1, 96, 0.2)
        for s in range(n_snap):
            if s:
                eng.verlet_steps(5)
            _take(eng, m)
        _assert_equals_model(eng, m, n)
        assert eng.vanhove_profile()["origins_live"] == max_lag
    assert m.H[max_lag, 96] > 0 and m.H[:, 1:96].sum() > 0


# ---- 3. identity across re-sorts -------------------------------------------------------------------------------------
def test_identity_across_resorts(monkeypatch):
    """a re-sort every 3 steps falls between every two snapshots 5 steps apart: a term must pair a particle with
    itself, whatever slot it is in.  A slot-paired histogram pairs particles up to a box apart: all overflow."""
    monkeypatch.setenv("LJMD_RESORT_EVERY", "3")
    n, max_lag = 2048, 6
    p, r, v = synthetic.make_config(n, seed=12)
    m = VanHoveModel(max_lag, 1, 128, 1.0)
    with Engine(p) as eng:
        _start(eng, r, v)
        eng.vanhove_configure(max_lag, 1, 128, 1.0)
        _take(eng, m)
        for _ in range(11):
            eng.verlet_steps(5)
            _take(eng, m)
        hist, _, counts = _assert_equals_model(eng, m, n)
    assert np.array_equal(counts, tcf_model.reference_counts(12, max_lag, 1))
    assert hist[max_lag, 128] == 0                            # nobody moves 1 sigma in 30 steps of dt = 0.005


# ---- 4. no disturbance; S2 is the MSD sum ----------------------------------------------------------------------------
MODES = {"fp64": _lib.PRECISION_FP64, "reproducible": _lib.PRECISION_FP64_REPRODUCIBLE, "mixed": _lib.PRECISION_FP32_FORCE}


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


@pytest.mark.parametrize("mode, n", [("fp64", 2048), ("reproducible", 2048), ("mixed", 16384)])
def test_accumulates_leave_everything_else_bitwise_alone(mode, n, monkeypatch):
    """two engines run the same enqueued segments with g(r), MSD / VACF, the pressure tensor and the heat flux
    accumulated between them, one of them with van Hove accumulates enqueued back to back in between as well, across
    re-sorts: r, ru, v, a, the step records and the four other observables' results are bitwise equal.  With the same
    (max_lag, stride) on the same handle S2 is the MSD sum of ljmd_tcf_*, integer for integer, and the counts agree."""
    monkeypatch.setenv("LJMD_RESORT_EVERY", "3")
    seg, nseg, max_lag = 5, 4, 3
    p, r, v = synthetic.make_config(n, seed=11)
    out = []
    for with_vanhove in (False, True):
        with Engine(p, precision_mode=MODES[mode]) as eng:
            _start(eng, r, v)
            eng.rdf_configure(50)
            eng.tcf_configure(max_lag, 1)
            eng.stress_configure(nseg)
            eng.heatflux_configure(nseg)
            if with_vanhove:
                eng.vanhove_configure(max_lag, 1, 64, 0.1)
            for _ in range(nseg):
                eng.enqueue_steps(seg)
                eng.rdf_accumulate()
                if with_vanhove:
                    eng.vanhove_accumulate()
                eng.tcf_accumulate()
                eng.stress_accumulate()
                eng.heatflux_accumulate()
            scalars = np.stack(eng.collect_steps(seg * nseg))
            state = eng.get_state()
            others = (eng.rdf_read(), eng.tcf_read_exact(), eng.stress_read_exact(raw=True), eng.heatflux_read_exact(raw=True))
            vh = eng.vanhove_read_exact() if with_vanhove else None
        out.append((scalars, state, others, vh))
    (sc0, st0, ot0, _), (sc1, st1, ot1, vh) = out
    assert sc0.tobytes() == sc1.tobytes()
    for key in ("r", "ru", "v", "a"):
        for a, b in zip(st0[key], st1[key]):
            assert a.tobytes() == b.tobytes(), key
    _same(ot0, ot1)
    hist, sums, counts, snaps = vh
    tcf_sums, tcf_counts, tcf_snaps = ot1[1]
    assert snaps == tcf_snaps == nseg and np.array_equal(counts, tcf_counts)
    assert list(sums[S2]) == list(tcf_sums[tcf_model.MSD]) and int(sums[S2][max_lag]) > 0
    assert np.array_equal(hist.sum(axis=1), np.uint64(n) * counts.astype(np.uint64))


# ---- 5. ring wrap, many slices ---------------------------------------------------------------------------------------
def test_ring_wrap_and_many_slices():
    """max_lag = 511 with stride 1: 512 ring slots, every one reused; 511 live origins and the lag-0 row"""
    n, max_lag, n_snap, nbins = 64, 511, 520, 32
    p, r, v = synthetic.make_config(n, seed=61)
    m = VanHoveModel(max_lag, 1, nbins, 2.0)
    with Engine(p) as eng:
        _start(eng, r, v)
        eng.vanhove_configure(max_lag, 1, nbins, 2.0)
        for s in range(n_snap):
            if s:
                eng.verlet_steps(1)
            _take(eng, m)
        _, _, counts = _assert_equals_model(eng, m, n)
        assert eng.vanhove_profile()["origins_live"] == max_lag
    assert np.array_equal(counts, tcf_model.reference_counts(n_snap, max_lag, 1))


# ---- 6. trajectories -------------------------------------------------------------------------------------------------
def test_trajectories_reset_reconfigure_off_and_destroy():
    n, max_lag, stride, nbins, rmax = 500, 3, 1, 40, 0.08
    p, r, v = synthetic.make_config(n, seed=71)
    lib = _lib.load()
    m = VanHoveModel(max_lag, stride, nbins, rmax)
    with Engine(p) as eng:
        _start(eng, r, v)
        eng.vanhove_configure(max_lag, stride, nbins, rmax)
        for s in range(3):
            if s:
                eng.verlet_steps(4)
            _take(eng, m)
        first_h, first, counts = _assert_equals_model(eng, m, n)

        st = eng.get_state(("ru", "a"))                       # these leave everything alone
        eng.set_unwrapped(*st["ru"])
        eng.set_accel(*st["a"])
        eng.set_tail_corrections(True)
        eng.rdf_configure(20)
        eng.rdf_accumulate()
        eng.tcf_configure(2)
        eng.tcf_accumulate()
        eng.tcf_reset()
        eng.stress_configure(2)
        eng.stress_accumulate()
        eng.heatflux_configure(2)
        eng.heatflux_accumulate()
        eng.migrate()                                         # a no-op on one rank
        same_h, same, counts2, snaps = eng.vanhove_read_exact()
        assert snaps == 3 and np.array_equal(same, first) and np.array_equal(counts2, counts) and np.array_equal(same_h, first_h)
        eng.verlet_steps(4)
        _take(eng, m)                                         # the origins are still there
        _assert_equals_model(eng, m, n)

        eng.set_state(r[0], r[1], r[2], v[0], v[1], v[2])     # a new trajectory: origins dropped, sums and counts kept
        before_h, before, counts, snaps = eng.vanhove_read_exact()
        assert snaps == 4 and list(before[S2]) == m.S[S2] and np.array_equal(counts, m.counts) and np.array_equal(before_h, m.H)
        eng.compute_forces()
        m.new_trajectory()
        _take(eng, m)                                         # no origin is live: nothing added
        same_h, same, counts2, snaps = eng.vanhove_read_exact()
        assert snaps == 5 and np.array_equal(same, before) and np.array_equal(counts2, counts) and np.array_equal(same_h, before_h)
        eng.verlet_steps(4)
        _take(eng, m)
        _, more, _ = _assert_equals_model(eng, m, n)          # both trajectories average together
        assert not np.array_equal(more, before)

        eng.vanhove_reset()
        hist, sums, counts, snaps = eng.vanhove_read_exact()
        assert snaps == 0 and not counts.any() and not any(sums.ravel()) and not hist.any()
        m.reset()
        _take(eng, m)                                         # numbering restarted: snapshot 0 meets nothing
        eng.verlet_steps(2)
        _take(eng, m)
        _assert_equals_model(eng, m, n)

        eng.vanhove_configure(5, 2, 7, 0.5)                   # reconfigure: new shape, zeroed
        hist, sums, counts, snaps = eng.vanhove_read_exact()
        assert snaps == 0 and sums.shape == (2, 6) and hist.shape == (6, 8) and counts.shape == (6,)
        assert not counts.any() and not any(sums.ravel()) and not hist.any()
        eng.vanhove_configure(0)                              # off
        assert lib.ljmd_vanhove_read(eng._h, None, None, None, None, None) == _lib.LJMD_ERR_STATE
        assert lib.ljmd_vanhove_accumulate(eng._h) == _lib.LJMD_ERR_STATE
        eng.verlet_steps(2)
        eng.vanhove_configure(4, 1, 16, 0.1)                  # destroyed while configured, launches in flight
        eng.vanhove_accumulate()
        eng.verlet_steps(1)
        eng.vanhove_accumulate()


# ---- 7. range --------------------------------------------------------------------------------------------------------
def test_range_word_is_sticky_until_reset():
    """one coordinate at 2000: r2 = 4e6 < 2^40 but r4 = 1.6e13 >= 2^40 -- an arithmetic flag, nothing faults; the
    particle counts in the overflow column and enters both sums as 0"""
    n, nbins, rmax = 108, 16, 0.2
    p, r, v = synthetic.make_config(n, seed=81)
    m = VanHoveModel(4, 1, nbins, rmax)
    with Engine(p) as eng:
        _start(eng, r, v)
        eng.vanhove_configure(4, 1, nbins, rmax)
        _take(eng, m)
        ru = [a.copy() for a in eng.get_state(("ru",))["ru"]]
        ru[1][5] = 2000.0
        eng.set_unwrapped(*ru)
        _take(eng, m)
        assert m.range_flag and m.H[1, nbins] == 1 and m.H[1].sum() == n
        for read in (eng.vanhove_read, eng.vanhove_read_exact):
            with pytest.raises(LjmdError) as ei:
                read()
            assert ei.value.code == _lib.LJMD_ERR_RANGE and ei.value.message.startswith("ljmd_vanhove_read"), ei.value.message
        # the counts behind the flag are the model's: the library fills the caller's arrays before it reports the flag
        hist = np.zeros((5, nbins + 1), dtype=np.uint64)
        words = np.zeros((2, 5, 3), dtype=np.int64)
        lib = _lib.load()
        assert lib.ljmd_vanhove_read_exact(eng._h, hist.ctypes.data_as(_lib.C.POINTER(_lib.C.c_uint64)),
                                           words.ctypes.data_as(_lib.c_int64_p), None, None) == _lib.LJMD_ERR_RANGE
        assert np.array_equal(hist, m.H)
        u = words.view(np.uint64)
        for kind in (S2, S4):
            assert [(int(words[kind, l, 2]) << 128) + (int(u[kind, l, 1]) << 64) + int(u[kind, l, 0]) for l in range(5)] == m.S[kind]
        eng.verlet_steps(4)                                   # the handle still steps: not poisoned
        with pytest.raises(LjmdError) as ei:                  # sticky
            eng.vanhove_read()
        assert ei.value.code == _lib.LJMD_ERR_RANGE
        eng.vanhove_reset()
        _start(eng, r, v)                                     # sound unwrapped coordinates again
        m = VanHoveModel(4, 1, nbins, rmax)
        _take(eng, m)
        eng.verlet_steps(2)
        _take(eng, m)
        _assert_equals_model(eng, m, n)
        assert eng.vanhove_read()[4] == 2


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
        assert lib.ljmd_vanhove_accumulate(eng._h) == _lib.LJMD_ERR_STATE            # before configure
        assert "ljmd_vanhove_accumulate: the van Hove function is not configured" in _lib.last_error()
        assert lib.ljmd_vanhove_read(eng._h, None, None, None, None, None) == _lib.LJMD_ERR_STATE
        assert lib.ljmd_vanhove_read_exact(eng._h, None, None, None, None) == _lib.LJMD_ERR_STATE
        assert lib.ljmd_vanhove_reset(eng._h) == _lib.LJMD_ERR_STATE
        assert lib.ljmd_vanhove_profile_read(eng._h, None, None) == _lib.LJMD_ERR_STATE
        assert "ljmd_vanhove_profile_read: the van Hove function is not configured" in _lib.last_error()
        eng.vanhove_configure(3, 1, 10, 0.5)                                         # without a state
        code, msg = _code(eng.vanhove_accumulate)
        assert code == _lib.LJMD_ERR_STATE and "no state" in msg
        eng.set_state(r[0], r[1], r[2], v[0], v[1], v[2])
        code, msg = _code(eng.vanhove_accumulate)
        assert code == _lib.LJMD_ERR_STATE and "accelerations" in msg
        eng.compute_forces()
        for bad, text in (((-1, 1, 10, 0.5), "ljmd_vanhove_configure: max_lag = -1"),
                          ((4097, 16, 10, 0.5), "ljmd_vanhove_configure: max_lag = 4097"),
                          ((3, 0, 10, 0.5), "ljmd_vanhove_configure: origin_stride"),
                          ((3, -2, 10, 0.5), "ljmd_vanhove_configure: origin_stride"),
                          ((512, 1, 10, 0.5), "ljmd_vanhove_configure: max_lag / origin_stride + 1 = 513"),
                          ((1024, 2, 10, 0.5), "ljmd_vanhove_configure: max_lag / origin_stride + 1 = 513"),
                          ((3, 1, 0, 0.5), "ljmd_vanhove_configure: nbins = 0"),
                          ((3, 1, 4097, 0.5), "ljmd_vanhove_configure: nbins = 4097"),
                          ((3, 1, 10, 0.0), "ljmd_vanhove_configure: rmax"),
                          ((3, 1, 10, -1.0), "ljmd_vanhove_configure: rmax"),
                          ((3, 1, 10, float("inf")), "ljmd_vanhove_configure: rmax"),
                          ((3, 1, 10, float("nan")), "ljmd_vanhove_configure: rmax"),
                          ((512, 1, 0, 0.0), "ljmd_vanhove_configure: max_lag / origin_stride"),   # the order of the guards
                          ((3, 1, 0, 0.0), "ljmd_vanhove_configure: nbins")):
            code, msg = _code(lambda: eng.vanhove_configure(*bad))
            assert code == _lib.LJMD_ERR_INVALID_ARG and msg.startswith(text), msg
        hist, sums, counts, snaps = eng.vanhove_read_exact()                         # the refused calls changed nothing
        assert snaps == 0 and sums.shape == (2, 4) and hist.shape == (4, 11) and not counts.any() and not hist.any()
        assert eng.vanhove_profile() == {"kernel_ms": 0.0, "origins_live": 0}

        eng.step_begin()                                                             # inside a split-phase step
        code, msg = _code(eng.vanhove_accumulate)
        assert code == _lib.LJMD_ERR_STATE and "split-phase" in msg
        eng.step_finish()
        assert eng.vanhove_read_exact()[3] == 0

        m = VanHoveModel(3, 1, 10, 0.5)
        _take(eng, m)
        eng.verlet_steps(2)
        _take(eng, m)
        first_h, first, counts = _assert_equals_model(eng, m, n)
        again_h, again, counts2, snaps = eng.vanhove_read_exact()                    # read clears nothing
        assert snaps == 2 and np.array_equal(again, first) and np.array_equal(counts2, counts) and np.array_equal(again_h, first_h)
        assert lib.ljmd_vanhove_read(eng._h, None, None, None, None, None) == _lib.LJMD_OK     # every pointer may be NULL
        assert lib.ljmd_vanhove_read_exact(eng._h, None, None, None, None) == _lib.LJMD_OK
        assert lib.ljmd_vanhove_profile_read(eng._h, None, None) == _lib.LJMD_OK
        assert eng.vanhove_profile()["origins_live"] == 1


@pytest.mark.parametrize("kw", [{"devices": [0, 0]}, {"rank": 0, "n_ranks": 2}])
def test_rank_engines_and_multi_device_handles_are_refused(kw):
    n = 1024
    p, r, v = synthetic.make_config(n, seed=95)
    lib = _lib.load()
    with Engine(p, **kw) as eng:
        eng.set_state(r[0], r[1], r[2], v[0], v[1], v[2])
        code, msg = _code(lambda: eng.vanhove_configure(4, 1, 16, 0.5))
        assert code == _lib.LJMD_ERR_INVALID_ARG and msg.startswith("ljmd_vanhove_configure: n_ranks = 2"), msg
        assert "one-rank engine" in msg
        for rc in (lib.ljmd_vanhove_accumulate(eng._h), lib.ljmd_vanhove_read(eng._h, None, None, None, None, None),
                   lib.ljmd_vanhove_read_exact(eng._h, None, None, None, None), lib.ljmd_vanhove_reset(eng._h),
                   lib.ljmd_vanhove_profile_read(eng._h, None, None)):
            assert rc == _lib.LJMD_ERR_STATE and "not configured" in _lib.last_error()
        eng.vanhove_configure(0)                                                     # off is accepted anywhere
