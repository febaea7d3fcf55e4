"""-m gpu: the tile walk of rdf_pairs_kernel, stress_pairs_kernel and heatflux_pairs_kernel beyond one step per slice.

rdf_plan_walk gives every system below n ~ 16 000 slices of ONE column-tile step, so the 64-lane ballot block of the three
kernels (one copy, rdf_walk_tiles of csrc/ljmd_rdf.h) runs with one valid lane in every other test that pins them to a
reference.  LJMD_WALK_CHUNK sets the steps per slice: here the blocks have many live lanes, a slice has a second block, a
partial last block, the tie step and the wrap of the unordered walk and the own tile of the ordered walk fall into a later
block -- at sizes whose exact reference is affordable.  Every comparison is integer equality: the g(r) counts with
oracle.rdf_histogram_np, the 12 stress words with stress_model.words, the 9 heat-flux words with heatflux_model.words, all
on the state get_state returns; one reference per state, one engine run per knob value.  The heat flux exists on one-rank
engines only (cases A and W); whenever it is measured, the pressure tensor is accumulated on the same engine and the two
walks must have visited the same number of tile pairs: they skip by the same bound on the same boxes.

  case A  one rank, n = 8200: T = 132 tiles, U = 67 steps, the tie step u = 66
  case W  one rank, n = 2100 at rc = 0.49 L: T = 36 (33 live tiles, the last with 52 particles, 3 of padding only), U = 19,
          the tie step u = 18; one block of 19 live lanes, and slices of 7, 7 and 5 steps with the tie in the short one
  case B  devices [0, 0], n = 4400: TB = 36, T = U = 72; rank 1 meets its own tiles I >= 64 in the second block
  case C  devices [0, 0, 0, 0], n = 4096: T = U = 64, one full block and no tail
  case D  two rank engines, n = 4400, the test performing the exchange: partials that differ and add up
a heat-flux series across slices (the workgroups' partial rows are never cleared between accumulates), two runs at
n = 131 072 with the knob unset (129 steps per slice on one rank, 64 on four), where the one-rank and the four-rank walk
must agree with each other, with the stateless g(r) kernel and with the engine's own virial, and the heat flux at that size
with the planner's slices against slices of 1 and of 64 steps."""
import functools
import hashlib

import numpy as np
import pytest

import heatflux_model
import stress_model
from ljmd_amd import Engine, analysis, md_types, synthetic

pytestmark = pytest.mark.gpu

NBINS = 125
CASES = {
    "A": dict(n=8200, devices=None, T=132, chunks=(None, 2, 33, 64, 65, 66, 67, 1000)),
    "B": dict(n=4400, devices=[0, 0], T=72, chunks=(None, 64, 65, 71, 72)),
    "C": dict(n=4096, devices=[0, 0, 0, 0], T=64, chunks=(64,)),
    "W": dict(n=2100, devices=None, T=36, chunks=(None, 19, 7)),
}
WHATS = ("rdf", "stress", "heatflux")


def _cases(cases, whats=WHATS):
    """(case, what) pairs: the heat flux is refused on multi-device handles, so it joins the one-rank cases only"""
    return [(c, w) for c in cases for w in whats if w != "heatflux" or CASES[c]["devices"] is None]


# ---- states and their references --------------------------------------------------------------------------------------
_STATES = {}


def _key(r, v, L):
    """registers a state under the hash of its bytes: the references below are cached per state"""
    r, v = np.ascontiguousarray(r), np.ascontiguousarray(v)
    key = hashlib.sha256(r.tobytes() + v.tobytes() + np.float64(L).tobytes()).hexdigest()
    _STATES.setdefault(key, (r.copy(), v.copy(), float(L)))
    return key


@functools.lru_cache(maxsize=None)
def _model_words(key, rc):
    r, v, L = _STATES[key]
    words, flag = stress_model.words(r, v, L, rc)
    assert not flag
    return tuple(words)


@functools.lru_cache(maxsize=None)
def _heatflux_words(key, rc):
    r, v, L = _STATES[key]
    words, flag = heatflux_model.words(r, v, L, rc)
    assert not flag
    return tuple(words)


@functools.lru_cache(maxsize=None)
def _oracle_hist(key, rmax):
    from oracle import oracle as O
    r, _v, L = _STATES[key]
    h = np.zeros(NBINS, dtype=np.uint64)
    O.rdf_histogram_np(r[0].copy(), r[1].copy(), r[2].copy(), L, NBINS, rmax, h)
    h.setflags(write=False)
    return h


@functools.lru_cache(maxsize=None)
def _config(n):
    p, r, v = synthetic.make_config(n, seed=7000 + n)
    return p.box_length, p.dt, r, v


def _input(n, kind):
    """kind 'compact': the synthetic configuration in [0, L).  'spread': a subset shifted by +-2 L, the spread above the
    2.4 L below which the handle knows its positions compact: nothing is skipped, every bit of a ballot is set.  'face': a
    subset shifted by +L only: spread ~2 L, skipping stays on and the tile boxes span a face of the box"""
    L, dt, r, v = _config(n)
    r = r.copy()
    if kind == "spread":
        r[0, ::5] += 2 * L
        r[1, 1::7] -= 2 * L
        r[2, 2::11] += 2 * L
    elif kind == "face":
        r[0, ::3] += L
        r[1, 1::4] += L
        r[2, 2::5] += L
    else:
        assert kind == "compact"
    return L, dt, r, v


def _set_chunk(monkeypatch, chunk):
    if chunk is None:
        monkeypatch.delenv("LJMD_WALK_CHUNK", raising=False)
    else:
        monkeypatch.setenv("LJMD_WALK_CHUNK", str(chunk))


def _measure(eng, what, rcut):
    """one accumulate of the kernel `what` on the resident state -> (counts or words, profile)"""
    if what == "rdf":
        eng.rdf_configure(NBINS, rcut)
        eng.rdf_accumulate()
        hist, count = eng.rdf_read()
        assert count == 1 and hist.shape == (NBINS,)
        return hist, eng.rdf_profile()
    eng.stress_configure(1)
    eng.stress_accumulate()
    words = eng.stress_read_exact()
    assert words.shape == (1, 12)
    if what == "stress":
        return tuple(words[0]), eng.stress_profile()
    # the heat flux beside the pressure tensor of the same state at the same rc: the two kernels' walks skip by the
    # same bound (rc2 (1 + 1e-10), rdf_tile_gap2) on the same boxes, so they visit the same tile pairs
    assert what == "heatflux"
    eng.heatflux_configure(1)
    eng.heatflux_accumulate()
    words = eng.heatflux_read_exact()
    assert words.shape == (1, 9)
    prof, sprof = eng.heatflux_profile(), eng.stress_profile()
    prof["stress_walk"] = (sprof["tile_pairs_total"], sprof["tile_pairs_visited"])
    return tuple(words[0]), prof


def _walks_agree(prof):
    """the heat flux's tile-pair counts against those of the pressure tensor accumulated beside it (_measure)"""
    return "stress_walk" not in prof or prof["stress_walk"] == (prof["tile_pairs_total"], prof["tile_pairs_visited"])


def _want(what, r, v, L, rcut):
    key = _key(r, v, L)
    return {"rdf": _oracle_hist, "stress": _model_words, "heatflux": _heatflux_words}[what](key, rcut)


def _same(what, got, want):
    return np.array_equal(got, want) if what == "rdf" else got == want


def _sweep(monkeypatch, what, case, kind, rcut, steps=0, chunks=None):
    """the engine of `case` on the state `kind`, once per knob value, against the one reference of the state; the
    tile-pair counts of the profile must not depend on the knob -> (tile_pairs_total, tile_pairs_visited)"""
    c = CASES[case]
    L, dt, r, v = _input(c["n"], kind)
    p = md_types.init_params(c["n"], L, dt, rcut)               # the stress cutoff is the engine's rc
    if kind == "spread" and c["devices"] is not None:
        monkeypatch.setenv("LJMD_N3", "0")                      # the multi-rank Newton-3 force kernel wants wrapped positions
    profiles = {}
    for chunk in (c["chunks"] if chunks is None else chunks):
        _set_chunk(monkeypatch, chunk)
        kw = {} if c["devices"] is None else {"devices": c["devices"]}
        with Engine(p, **kw) as eng:
            eng.set_state(r[0], r[1], r[2], v[0], v[1], v[2])
            eng.compute_forces()
            if steps:
                eng.verlet_steps(steps)
            got, prof = _measure(eng, what, rcut)
            st = eng.get_state(("r", "v"))
        r1, v1 = np.stack(st["r"]), np.stack(st["v"])
        if not steps:
            assert r1.tobytes() == r.tobytes() and v1.tobytes() == v.tobytes()
        want = _want(what, r1, v1, L, rcut)
        assert _same(what, got, want), (what, case, kind, "LJMD_WALK_CHUNK", chunk)
        assert _walks_agree(prof), (what, case, kind, "LJMD_WALK_CHUNK", chunk, prof)
        profiles[chunk] = prof
    totals = {(q["tile_pairs_total"], q["tile_pairs_visited"]) for q in profiles.values()}
    assert len(totals) == 1, {k: (q["tile_pairs_total"], q["tile_pairs_visited"]) for k, q in profiles.items()}
    total, visited = totals.pop()
    print("%s case %s %s rc = %.4f: tile pairs visited %d of %d" % (what, case, kind, rcut, visited, total))
    T = c["T"]
    assert total == (T * (T // 2) + T // 2 if c["devices"] is None else T * T), (total, T)
    assert 0 < visited <= total
    return total, visited


# ---- 1. the knob values of cases A, B, C ------------------------------------------------------------------------------
@pytest.mark.parametrize("case, what", _cases("ABC"))
def test_compact_state_sparse_ballots(monkeypatch, what, case):
    """rc = rmax = 2.5: the boxes keep a sparse subset of the valid lanes"""
    total, visited = _sweep(monkeypatch, what, case, "compact", 2.5)
    assert visited < total


@pytest.mark.parametrize("case, what", _cases("ABC"))
def test_spread_state_full_ballots(monkeypatch, what, case):
    """positions not known to be compact: nothing is skipped, every valid lane's bit is set"""
    c = CASES[case]
    L, _dt, r, _v = _input(c["n"], "spread")
    assert min(np.ptp(r[k]) for k in range(3)) > 2.4 * L
    total, visited = _sweep(monkeypatch, what, case, "spread", 2.5)
    assert visited == total


@pytest.mark.parametrize("what", ["rdf", "stress"])
def test_case_b_at_a_wide_cutoff(monkeypatch, what):
    """rc = rmax = 0.49 L: nearly half of all pairs are inside"""
    L = _config(CASES["B"]["n"])[0]
    _sweep(monkeypatch, what, "B", "compact", 0.49 * L)


@pytest.mark.parametrize("what", WHATS)
def test_case_a_after_steps_across_re_sorts(monkeypatch, what):
    """25 steps with a re-sort every 3, then one slice of all 67 steps: the slot order is the engine's own"""
    monkeypatch.setenv("LJMD_RESORT_EVERY", "3")
    total, visited = _sweep(monkeypatch, what, "A", "compact", 2.5, steps=25, chunks=(67,))
    assert visited < total


@pytest.mark.parametrize("case, chunks, what", [
    pytest.param(case, chunks, what, id="%s-chunks%d-%s" % (case, k, what))
    for k, (case, chunks) in enumerate([("A", (None, 65, 67)), ("B", (None, 65, 72))]) for _c, what in _cases(case)])
def test_state_spanning_a_box_face_keeps_skipping(monkeypatch, what, case, chunks):
    """raw input with a subset shifted by +L: still compact (spread ~2 L < 2.4 L), so the walk skips by boxes that span a
    face of the periodic box"""
    c = CASES[case]
    L, _dt, r, _v = _input(c["n"], "face")
    assert 1.5 * L < max(np.ptp(r[k]) for k in range(3)) < 2.4 * L
    total, visited = _sweep(monkeypatch, what, case, "face", 2.5, chunks=chunks)
    assert visited < total


@pytest.mark.parametrize("what", ["stress", "heatflux"])
def test_case_w_wide_cutoff_many_live_lanes(monkeypatch, what):
    """rc = 0.49 L at n = 2100: nearly every tile pair is kept, so a block of 19 valid lanes has (nearly) 19 set bits and
    the bit loop runs that often per ballot; with 7 steps per slice the tie step is the last of a slice of 5"""
    L = _config(CASES["W"]["n"])[0]
    total, visited = _sweep(monkeypatch, what, "W", "compact", 0.49 * L)
    assert total == 36 * 18 + 18


# ---- 1b. a heat-flux series across slices -------------------------------------------------------------------------------
def test_heatflux_series_across_slices(monkeypatch):
    """d_part, d_pcount and d_pflag are never cleared: every workgroup of the (row blocks, slices) grid rewrites its own
    rows on every accumulate, also a slice in which nothing was visited.  Three accumulates 5 steps apart at 7 steps per
    slice (slices of 7, 7 and 5 of the 19 steps) with a re-sort every 2 steps, each row against the model of its own state;
    after a reset row 0 is the current state's; and an engine with the knob unset returns the same rows for the states"""
    n, rc = 2100, 2.5
    L, dt, r, v = _input(n, "compact")
    p = md_types.init_params(n, L, dt, rc)
    monkeypatch.setenv("LJMD_RESORT_EVERY", "2")
    _set_chunk(monkeypatch, 7)
    states = []
    with Engine(p) as eng:
        eng.set_state(r[0], r[1], r[2], v[0], v[1], v[2])
        eng.compute_forces()
        eng.heatflux_configure(4)
        for k in range(3):
            if k:
                eng.verlet_steps(5)
            eng.heatflux_accumulate()
            st = eng.get_state(("r", "v"))
            states.append((np.stack(st["r"]), np.stack(st["v"])))
        rows = eng.heatflux_read_exact()
        eng.heatflux_reset()
        eng.heatflux_accumulate()
        again = eng.heatflux_read_exact()
        prof = eng.heatflux_profile()
    want = [_want("heatflux", r1, v1, L, rc) for r1, v1 in states]
    assert len(set(want)) == 3 and all(w != 0 for row in want for w in row)
    assert rows.shape == (3, 9) and again.shape == (1, 9)
    for k in range(3):
        assert tuple(rows[k]) == want[k], ("LJMD_WALK_CHUNK = 7, snapshot", k)
    assert tuple(again[0]) == want[2]
    print("heatflux series n = %d: tile pairs visited %d of %d" % (n, prof["tile_pairs_visited"], prof["tile_pairs_total"]))
    assert 0 < prof["tile_pairs_visited"] < prof["tile_pairs_total"] == 36 * 18 + 18
    _set_chunk(monkeypatch, None)
    with Engine(p) as eng:
        eng.heatflux_configure(4)
        for r1, v1 in states:
            eng.set_state(r1[0], r1[1], r1[2], v1[0], v1[1], v1[2])
            eng.compute_forces()
            eng.heatflux_accumulate()
        other = eng.heatflux_read_exact()
    assert other.shape == (3, 9)
    for k in range(3):
        assert tuple(other[k]) == want[k], ("LJMD_WALK_CHUNK unset, snapshot", k)


# ---- 2. case D: rank engines ------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("what", ["rdf", "stress"])
def test_rank_engines_partials_differ_and_add_up(monkeypatch, what):
    """two rank engines (n_ranks = 2) on one card, each walking its 36 row tiles over all 72 steps in one slice"""
    monkeypatch.setenv("LJMD_N3_MIN_N", "100000000")          # gather kernels: no force exchange to emulate
    monkeypatch.setenv("LJMD_WALK_CHUNK", "72")
    n = CASES["B"]["n"]
    L, dt, r, v = _input(n, "compact")
    p = md_types.init_params(n, L, dt, 2.5)
    engines = [Engine(p, rank=g, n_ranks=2) for g in range(2)]
    try:
        for e in engines:
            e.set_state(r[0], r[1], r[2], v[0], v[1], v[2])
        _emulated_allgather(engines)
        for e in engines:
            e.forces_partial()
        parts, profs = [], []
        for e in engines:
            got, prof = _measure(e, what, 2.5)
            parts.append(got)
            profs.append(prof)
        shards = [e.get_state(("r", "v")) for e in engines]
    finally:
        for e in engines:
            e.close()
    r1 = np.concatenate([np.stack(s["r"]) for s in shards], axis=1)
    v1 = np.concatenate([np.stack(s["v"]) for s in shards], axis=1)
    want = _want(what, r1, v1, L, 2.5)
    assert not _same(what, parts[0], parts[1])
    total = parts[0] + parts[1] if what == "rdf" else tuple(a + b for a, b in zip(*parts))
    assert _same(what, total, want)
    for prof in profs:
        assert prof["tile_pairs_total"] == 36 * 72 and 0 < prof["tile_pairs_visited"] < prof["tile_pairs_total"]


# ---- 3. the planner's own slices: n = 131 072, the knob unset ---------------------------------------------------------
# one rank: TB = T = 2048, U = 1025, 512 row blocks -> 8 slices of 129 steps (two full blocks and one lane);
# [0] * 4:  TB = 512, T = U = 2048, 128 row blocks -> 32 slices of 64 steps.
N_BIG = 131072
BIG_TOTALS = {"one": 2048 * 1024 + 1024, "four": 2048 * 2048}


def _big_engines(monkeypatch, p):
    monkeypatch.delenv("LJMD_WALK_CHUNK", raising=False)
    yield "one", Engine(p)
    yield "four", Engine(p, devices=[0, 0, 0, 0])


@pytest.mark.parametrize("rc", [2.5, None])
def test_natural_size_stress_one_rank_against_four(oracle, monkeypatch, rc):
    """The unordered walk at 129 steps per slice and the ordered walk at 64 are two forms at two slicings: integer sums
    depend on neither, so the 12 words are equal.  And the trace of the one-rank tensor agrees with the pressure formed
    from the engine's d_epot of the same state (tail off), within the bound of
    test_gpu_stress_resident.py::test_isotropic_pressure_against_the_oracle: 1e-13 relative on d_epot, through / (3 V)"""
    p, r, v = synthetic.make_config(N_BIG, seed=7000 + N_BIG)
    if rc is not None:
        p = md_types.init_params(N_BIG, p.box_length, p.dt, rc)
    words, pd, d_epot = {}, None, None
    for name, eng in _big_engines(monkeypatch, p):
        with eng:
            eng.set_tail_corrections(False)
            eng.set_state(r[0], r[1], r[2], v[0], v[1], v[2])
            _e, d, _dd = eng.compute_forces()
            words[name], prof = _measure(eng, "stress", p.rc)
            if name == "one":
                pd, d_epot = eng.stress_read()[0], d
            st = eng.get_state(("r", "v"))
        assert np.stack(st["r"]).tobytes() == r.tobytes() and np.stack(st["v"]).tobytes() == v.tobytes()
        assert prof["tile_pairs_total"] == BIG_TOTALS[name], (name, prof)
        assert 0 < prof["tile_pairs_visited"] <= prof["tile_pairs_total"]
        if rc is not None:
            assert prof["tile_pairs_visited"] < prof["tile_pairs_total"] // 4, (name, prof)
    assert words["one"] == words["four"], [c for c in range(12) if words["one"][c] != words["four"][c]]
    assert all(w != 0 for w in words["one"])
    po = oracle.derive_params(p.n, p.box_length, p.dt, p.rc)
    ekin = oracle.ekin_fused(v[0], v[1], v[2])
    _etot, _temp, press = oracle.observables(po, 0.0, ekin, d_epot)
    V = (p.box_length * p.box_length) * p.box_length
    iso = ((pd[0] + pd[1]) + pd[2]) / 3.0
    tol = 1e-13 * abs(d_epot) / (3.0 * V)
    print("n = %d, rc = %.4f: p_iso = %.15e, from d_epot %.15e, |diff| = %.3e, tolerance %.3e"
          % (N_BIG, p.rc, iso, press, abs(iso - press), tol))
    assert abs(iso - press) <= tol


@pytest.mark.parametrize("rmax_over_L, rmax", [(None, 2.5), (0.5, None)])
def test_natural_size_rdf_against_the_stateless_kernel(monkeypatch, rmax_over_L, rmax):
    """the resident counts of both handles equal ljmd_rdf_histogram's (pinned to the oracle by its own tests), the
    comparison of test_gpu_rdf_resident.py::test_mixed_precision_mode"""
    p, r, v = synthetic.make_config(N_BIG, seed=7000 + N_BIG)
    L = p.box_length
    rmax = rmax_over_L * L if rmax is None else rmax
    want = np.zeros(NBINS, dtype=np.uint64)
    analysis.rdf_histogram(r[0], r[1], r[2], L, NBINS, rmax, want)
    assert want.sum() > 0
    for name, eng in _big_engines(monkeypatch, p):
        with eng:
            eng.set_state(r[0], r[1], r[2], v[0], v[1], v[2])
            eng.compute_forces()
            hist, prof = _measure(eng, "rdf", rmax)
            x, y, z = eng.get_state(("r",))["r"]
        assert np.stack([x, y, z]).tobytes() == r.tobytes()
        assert np.array_equal(hist, want), (name, np.flatnonzero(hist != want)[:8])
        assert prof["tile_pairs_total"] == BIG_TOTALS[name], (name, prof)
        assert 0 < prof["tile_pairs_visited"] <= prof["tile_pairs_total"]


def test_natural_size_heatflux_across_slicings(monkeypatch):
    """No exact model is affordable at n = 131 072, but integer sums depend on no slicing: the 9 words of the planner's own
    8 slices of 129 steps (two full blocks and one lane) equal those of 1025 slices of one step -- the shape the small
    systems pin to the model -- and of slices of 64 steps, whole blocks with no tail.  Three engines, one accumulate each"""
    p, r, v = synthetic.make_config(N_BIG, seed=7000 + N_BIG)
    p = md_types.init_params(N_BIG, p.box_length, p.dt, 2.5)
    words, visited = {}, {}
    for chunk in (None, 1, 64):
        _set_chunk(monkeypatch, chunk)
        with Engine(p) as eng:
            eng.set_state(r[0], r[1], r[2], v[0], v[1], v[2])
            eng.compute_forces()
            words[chunk], prof = _measure(eng, "heatflux", p.rc)
            st = eng.get_state(("r", "v"))
        assert np.stack(st["r"]).tobytes() == r.tobytes() and np.stack(st["v"]).tobytes() == v.tobytes()
        assert prof["tile_pairs_total"] == BIG_TOTALS["one"], (chunk, prof)
        assert 0 < prof["tile_pairs_visited"] < prof["tile_pairs_total"] // 4, (chunk, prof)
        assert _walks_agree(prof), (chunk, prof)
        visited[chunk] = prof["tile_pairs_visited"]
    print("heatflux n = %d: tile pairs visited %d of %d" % (N_BIG, visited[None], BIG_TOTALS["one"]))
    assert len(words[None]) == 9 and all(w != 0 for w in words[None])
    for chunk in (1, 64):
        assert words[chunk] == words[None], (chunk, [c for c in range(9) if words[chunk][c] != words[None][c]])
        assert visited[chunk] == visited[None]
