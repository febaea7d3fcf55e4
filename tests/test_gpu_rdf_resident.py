"""-m gpu: g(r) of the resident system accumulated on the single / sharded engine (ljmd_rdf_*, Engine.rdf_*).  The counts
are integers: every comparison is equality with oracle.rdf_histogram_np (the reference's numpy arithmetic) on the
positions get_state returns."""
import numpy as np
import pytest

from ljmd_amd import Engine, _lib, analysis, md_types, synthetic
from ljmd_amd._lib import LjmdError

pytestmark = pytest.mark.gpu


def _oracle_hist(oracle, x, y, z, L, nbins, rmax):
    h = np.zeros(nbins, dtype=np.uint64)
    oracle.rdf_histogram_np(np.ascontiguousarray(x), np.ascontiguousarray(y), np.ascontiguousarray(z), L, nbins, rmax, h)
    return h


def _stateless_hist(x, y, z, L, nbins, rmax):
    h = np.zeros(nbins, dtype=np.uint64)
    analysis.rdf_histogram(np.ascontiguousarray(x), np.ascontiguousarray(y), np.ascontiguousarray(z), L, nbins, rmax, h)
    return h


def _start(eng, r, v):
    eng.set_state(r[0], r[1], r[2], v[0], v[1], v[2])
    eng.compute_forces()


def _one_shot(eng, nbins, rmax):
    eng.rdf_configure(nbins, rmax)
    eng.rdf_accumulate()
    hist, count = eng.rdf_read()
    assert count == 1 and hist.shape == (nbins,) and hist.dtype == np.uint64
    return hist


# ---- 1. one-shot counts ----------------------------------------------------------------------------------------------
# n = 2: one pair; 63 / 64 / 65: one tile not full, full, one particle in the second; 130: a third tile; 1000: the largest
# system the engine leaves in the caller's order; 4096: k-d ordered, 64 tiles.  (The slot count is padded to a multiple of
# 256, so the tile count is always a multiple of 4 and every system here has all-padding tiles but n = 4096.)
# rmax_over_L None = rmax given in sigma.
@pytest.mark.parametrize("n, nbins, rmax_over_L, rmax", [
    (2, 200, 0.5, None), (63, 200, 0.5, None), (64, 200, 0.5, None), (65, 200, 0.5, None), (130, 200, 0.5, None),
    (1000, 200, 0.5, None), (4096, 200, 0.5, None), (4096, 8192, 0.5, None), (4096, 200, None, 2.0),
    (500, 200, 0.8, None),
])
def test_one_shot_counts_equal_the_oracle(oracle, n, nbins, rmax_over_L, rmax):
    p, r, v = synthetic.make_config(n, seed=100 + n)
    L = p.box_length
    rmax = rmax_over_L * L if rmax is None else rmax
    with Engine(p) as eng:
        _start(eng, r, v)
        hist = _one_shot(eng, nbins, rmax)
        x, y, z = eng.get_state(("r",))["r"]
    want = _oracle_hist(oracle, x, y, z, L, nbins, rmax)
    assert np.array_equal(hist, want), (n, np.flatnonzero(hist != want)[:8])
    assert hist.sum() > 0 or n == 2
    if rmax >= 0.8 * L:
        assert hist.sum() > 0.9 * n * (n - 1)               # nearly every pair lies within 0.8 L of its nearest image


# ---- 2. ties ---------------------------------------------------------------------------------------------------------
def test_lattice_ties_on_bin_edges_and_half_box(oracle):
    """unjittered 4 x 4 x 4 simple-cubic lattice in L = 4 with rmax = 2, 8 bins: separations exactly on bin edges
    (r / dr an integer) and components with d / L = +-0.5 -- both true-division paths decide"""
    n, L, rmax, nbins = 64, 4.0, 2.0, 8
    p = md_types.init_params(n, L, 0.005, 1.9)
    g = np.arange(4, dtype=np.float64)
    site = np.stack([a.ravel() for a in np.meshgrid(g, g, g, indexing="ij")])             # [3, 64], integers
    for r in (site, site + 0.5):                                                          # corners / cell centres
        with Engine(p) as eng:
            _start(eng, r, np.zeros_like(r))
            hist = _one_shot(eng, nbins, rmax)
            x, y, z = eng.get_state(("r",))["r"]
        want = _oracle_hist(oracle, x, y, z, L, nbins, rmax)
        assert want[4] == 2 * 3 * 64 and want.sum() > want[4]                             # r = 1 sits on the edge of bin 4
        assert np.array_equal(hist, want), (hist, want)
        assert np.array_equal(hist, _stateless_hist(x, y, z, L, nbins, rmax))


# ---- 3. positions that are not compact -------------------------------------------------------------------------------
def test_raw_input_spanning_more_than_a_box(oracle):
    """raw set_state input with particles shifted by +-L and +-2 L: the handle does not know the positions to be compact,
    nothing is skipped, and the counts are those of the positions as given"""
    n, nbins = 4096, 100
    p, r, v = synthetic.make_config(n, seed=7)
    L = p.box_length
    r = r.copy()
    r[0, ::5] += L
    r[1, 1::7] -= L
    r[2, 2::11] += 2 * L
    r[0, 3::13] -= 2 * L
    with Engine(p) as eng:
        _start(eng, r, v)
        hist = _one_shot(eng, nbins, 2.0)
        prof = eng.rdf_profile()
        x, y, z = eng.get_state(("r",))["r"]
    assert np.ptp(x) > 2.4 * L
    assert np.array_equal(hist, _oracle_hist(oracle, x, y, z, L, nbins, 2.0))
    assert prof["tile_pairs_visited"] == prof["tile_pairs_total"] > 0


# ---- 4. during a run ---------------------------------------------------------------------------------------------------
def test_accumulation_between_enqueued_segments(oracle):
    """segments and accumulates enqueued back to back with no synchronisation, as md_simulation_gpu does; n = 2048
    re-sorts every 200 steps (LaunchPlan::resort_every), so the 250 steps cross a re-sort"""
    n, nbins, rmax, seg, nseg = 2048, 150, 2.5, 50, 5
    p, r, v = synthetic.make_config(n, seed=11)
    L = p.box_length
    with Engine(p) as ref:                                    # stepped synchronously, no g(r)
        _start(ref, r, v)
        want = np.zeros(nbins, dtype=np.uint64)
        ref_scalars = []
        for _ in range(nseg):
            ref_scalars.append(np.stack(ref.verlet_steps(seg)))
            x, y, z = ref.get_state(("r",))["r"]
            want += _oracle_hist(oracle, x, y, z, L, nbins, rmax)
        ref_state = ref.get_state()
    with Engine(p) as eng:
        _start(eng, r, v)
        eng.rdf_configure(nbins, rmax)
        for _ in range(nseg):
            eng.enqueue_steps(seg)
            eng.rdf_accumulate()
        scalars = np.stack(eng.collect_steps(seg * nseg))
        hist, count = eng.rdf_read()
        state = eng.get_state()
    assert count == nseg
    assert np.array_equal(hist, want), np.flatnonzero(hist != want)[:8]
    assert scalars.tobytes() == np.concatenate(ref_scalars, axis=1).tobytes()
    for key in ("r", "ru", "v", "a"):
        for got, exp in zip(state[key], ref_state[key]):
            assert got.tobytes() == exp.tobytes(), key


# ---- 5. ranks ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, devices", [(1024, [0, 0]), (4096, [0, 0, 0, 0])])
def test_multi_device_handle(oracle, n, devices):
    """the sum over the ranks of a multi-device handle equals the oracle's counts and those of a single handle given the
    same positions -- after 60 steps, and again after an ownership migration"""
    nbins = 120
    p, r, v = synthetic.make_config(n, seed=21)
    L = p.box_length
    rmax = 0.5 * L
    with Engine(p, devices=devices) as eng:
        _start(eng, r, v)
        eng.verlet_steps(60)
        hist = _one_shot(eng, nbins, rmax)
        prof = eng.rdf_profile()
        st = eng.get_state(("r", "v"))
        eng.migrate()
        eng.rdf_reset()
        eng.rdf_accumulate()
        after, count = eng.rdf_read()
        x2, y2, z2 = eng.get_state(("r",))["r"]
    x, y, z = st["r"]
    want = _oracle_hist(oracle, x, y, z, L, nbins, rmax)
    assert np.array_equal(hist, want), np.flatnonzero(hist != want)[:8]
    assert 0 < prof["tile_pairs_visited"] <= prof["tile_pairs_total"]
    assert count == 1 and np.array_equal(after, _oracle_hist(oracle, x2, y2, z2, L, nbins, rmax))
    with Engine(p) as one:
        _start(one, np.stack([x, y, z]), np.stack(st["v"]))
        assert np.array_equal(_one_shot(one, nbins, rmax), hist)


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


def test_rank_engines_return_partials_that_add_up(oracle, monkeypatch):
    """two rank engines (ljmd_create with n_ranks = 2) on one card, the test performing the exchanges: each returns the
    ordered pairs of its own rows, the two differ and add up; inside a split-phase step the call is refused"""
    monkeypatch.setenv("LJMD_N3_MIN_N", "100000000")          # gather kernels: no force exchange to emulate
    n, nbins = 2048, 90
    p, r, v = synthetic.make_config(n, seed=31)
    L = p.box_length
    rmax = 0.5 * L
    engines = [Engine(p, rank=g, n_ranks=2) for g in range(2)]
    try:
        for e in engines:
            e.set_state(r[0], r[1], r[2], v[0], v[1], v[2])
            e.rdf_configure(nbins, rmax)
        _emulated_allgather(engines)
        for e in engines:
            e.forces_partial()
        for _ in range(3):
            for e in engines:
                e.step_begin()
            for e in engines:
                with pytest.raises(LjmdError) as ei:
                    e.rdf_accumulate()
                assert ei.value.code == _lib.LJMD_ERR_STATE and "split-phase" in ei.value.message
            _emulated_allgather(engines)
            for e in engines:
                e.step_finish()
        parts = []
        for e in engines:
            e.rdf_accumulate()
            hist, count = e.rdf_read()
            assert count == 1
            parts.append(hist)
        xyz = [np.concatenate([e.get_state(("r",))["r"][ax] for e in engines]) for ax in range(3)]
    finally:
        for e in engines:
            e.close()
    assert not np.array_equal(parts[0], parts[1])
    assert np.array_equal(parts[0] + parts[1], _oracle_hist(oracle, xyz[0], xyz[1], xyz[2], L, nbins, rmax))


# ---- 6. precision modes ------------------------------------------------------------------------------------------------
def test_reproducible_mode(oracle):
    n, nbins = 500, 80
    p, r, v = synthetic.make_config(n, seed=41)
    L = p.box_length
    with Engine(p, precision_mode=_lib.PRECISION_FP64_REPRODUCIBLE) as eng:
        _start(eng, r, v)
        eng.verlet_steps(20)
        hist = _one_shot(eng, nbins, 0.5 * L)
        x, y, z = eng.get_state(("r",))["r"]
    assert np.array_equal(hist, _oracle_hist(oracle, x, y, z, L, nbins, 0.5 * L))


def test_mixed_precision_mode():
    """n = 16 384 is the smallest system of the mode; the oracle's numpy pass is too slow there, the stateless kernel
    (pinned to the oracle by its own tests) is the comparison"""
    n, nbins = 16384, 300
    p, r, v = synthetic.make_config(n, seed=43)
    L = p.box_length
    with Engine(p, precision_mode=_lib.PRECISION_FP32_FORCE) as eng:
        _start(eng, r, v)
        eng.verlet_steps(5)
        hist = _one_shot(eng, nbins, 0.5 * L)
        x, y, z = eng.get_state(("r",))["r"]
    assert hist.sum() > 0
    assert np.array_equal(hist, _stateless_hist(x, y, z, L, nbins, 0.5 * L))


# ---- 7. what the walk skips --------------------------------------------------------------------------------------------
def test_skip_accounting():
    """n = 4096 at rho = 0.8 (L = 17.2), k-d ordered right after set_state: 4 x 4 x 4 tiles of side L / 4 = 4.3 > rmax = 2,
    so only the 27 neighbours of a tile out of 64 can be within reach (0.42); with rmax = 0.9 L no pair of boxes can be
    proven farther apart (the minimum image is at most sqrt(3) L / 2 = 0.87 L away)"""
    n, nbins = 4096, 64
    p, r, v = synthetic.make_config(n, seed=51, rho=0.8)
    L = p.box_length
    with Engine(p) as eng:
        _start(eng, r, v)
        eng.rdf_configure(nbins, 2.0)
        eng.rdf_accumulate()
        near = eng.rdf_profile()
        eng.rdf_configure(nbins, 0.9 * L)
        eng.rdf_accumulate()
        far = eng.rdf_profile()
    T = 4096 // 64
    assert near["tile_pairs_total"] == far["tile_pairs_total"] == T * (T // 2) + T // 2     # unordered pairs + diagonal
    assert 0 < near["tile_pairs_visited"] <= 0.5 * near["tile_pairs_total"], near
    assert far["tile_pairs_visited"] == far["tile_pairs_total"], far
    assert near["kernel_ms"] > 0.0 and far["kernel_ms"] > 0.0


# ---- 8. sequence and guards --------------------------------------------------------------------------------------------
def _code(call):
    with pytest.raises(LjmdError) as ei:
        call()
    return ei.value.code, ei.value.message


def test_sequence_and_guards(oracle):
    n = 500
    p, r, v = synthetic.make_config(n, seed=61)
    L = p.box_length
    lib = _lib.load()
    with Engine(p) as eng:
        assert lib.ljmd_rdf_accumulate(eng._h) == _lib.LJMD_ERR_STATE                # before configure
        assert lib.ljmd_rdf_read(eng._h, None, None) == _lib.LJMD_ERR_STATE
        assert lib.ljmd_rdf_reset(eng._h) == _lib.LJMD_ERR_STATE
        assert lib.ljmd_rdf_profile_read(eng._h, None, None, None) == _lib.LJMD_ERR_STATE
        eng.rdf_configure(50)                                                        # without a state
        code, msg = _code(eng.rdf_accumulate)
        assert code == _lib.LJMD_ERR_STATE and "no state" in msg
        eng.set_state(r[0], r[1], r[2], v[0], v[1], v[2])
        code, msg = _code(eng.rdf_accumulate)
        assert code == _lib.LJMD_ERR_STATE and "accelerations" in msg
        eng.compute_forces()
        for nbins in (-1, 8193):
            assert _code(lambda: eng.rdf_configure(nbins))[0] == _lib.LJMD_ERR_INVALID_ARG
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            code, msg = _code(lambda: eng.rdf_configure(50, bad))
            assert code == _lib.LJMD_ERR_INVALID_ARG and msg.startswith("ljmd_rdf_configure: rmax"), msg
        hist, count = eng.rdf_read()                                                 # the refused calls changed nothing
        assert count == 0 and hist.shape == (50,) and not hist.any()
        assert eng.rdf_profile() == {"tile_pairs_visited": 0, "tile_pairs_total": 0, "kernel_ms": 0.0}

        eng.rdf_accumulate()
        once, count = eng.rdf_read()
        x, y, z = eng.get_state(("r",))["r"]
        assert count == 1 and np.array_equal(once, _oracle_hist(oracle, x, y, z, L, 50, 0.5 * L))
        eng.rdf_accumulate()
        twice, count = eng.rdf_read()
        assert count == 2 and np.array_equal(twice, 2 * once)
        again, count = eng.rdf_read()                                                # read clears nothing
        assert count == 2 and np.array_equal(again, twice)
        assert lib.ljmd_rdf_read(eng._h, None, None) == _lib.LJMD_OK                 # either pointer may be NULL
        eng.set_state(r[0], r[1], r[2], v[0], v[1], v[2])                            # set_state keeps the counts
        eng.set_accel(*eng.get_state(("a",))["a"])
        eng.set_tail_corrections(False)
        kept, count = eng.rdf_read()
        assert count == 2 and np.array_equal(kept, twice)
        eng.rdf_reset()
        zero, count = eng.rdf_read()
        assert count == 0 and not zero.any()

        eng.rdf_configure(75, 1.5)                                                   # reconfigure: new shape, zeroed
        fresh, count = eng.rdf_read()
        assert count == 0 and fresh.shape == (75,) and not fresh.any()
        eng.rdf_configure(0)                                                         # off
        assert lib.ljmd_rdf_read(eng._h, None, None) == _lib.LJMD_ERR_STATE
        assert lib.ljmd_rdf_accumulate(eng._h) == _lib.LJMD_ERR_STATE
        eng.rdf_configure(10)                                                        # destroyed while configured
        eng.rdf_accumulate()
