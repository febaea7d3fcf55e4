"""-m gpu: the batch engine in the reproducible mode (ljmd_batch_set_precision, LJMD_PRECISION_FP64_REPRODUCIBLE).  Per
replica the results are a function of the particle set alone: bitwise equal to the CPU model of the definition
(tests/reproducible_model.py) and to the single reproducible Engine, and bitwise independent of B, the slot, the
neighbours, the sampling interval, the launch grouping and the order of the particles inside the replica."""
import numpy as np
import pytest

import reproducible_model as M
from ljmd_amd import BatchEngine, Engine, _lib, init_params, synthetic
from ljmd_amd._lib import LjmdError
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

MODE = _lib.PRECISION_FP64_REPRODUCIBLE


def bits(x) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)


def assert_bitwise(a, b, what=""):
    ba, bb = bits(a), bits(b)
    assert ba.shape == bb.shape, what
    bad = np.flatnonzero(ba.ravel() != bb.ravel())
    assert bad.size == 0, (what, bad.size, np.ravel(a)[bad[:4]], np.ravel(b)[bad[:4]])


def _replicas(n, seeds, rc=None):
    """-> params, r[B, 3, n], v[B, 3, n]: distinct configurations of the same (n, L, dt, rc)"""
    cfg = [synthetic.make_config(n, seed=s) for s in seeds]
    p = cfg[0][0]
    if rc is not None:
        p = init_params(n, p.box_length, p.dt, rc)
    return p, np.stack([c[1] for c in cfg]), np.stack([c[2] for c in cfg])


def _set(eng, r, v):
    eng.set_state(r[:, 0], r[:, 1], r[:, 2], v[:, 0], v[:, 1], v[:, 2])


def _state(eng):
    """-> [B, 4, 3, n]: r, ru, v, a"""
    st = eng.get_state()
    return np.stack([np.stack(st[k], axis=1) for k in ("r", "ru", "v", "a")], axis=1)


# ---- 1. one force call against the model ------------------------------------------------------------------------------
def _force_case(n, seeds, rc_of_L=None, tail=True):
    p, r, v = _replicas(n, seeds)
    if rc_of_L is not None:
        p, r, v = _replicas(n, seeds, rc=rc_of_L * p.box_length)
    B = len(seeds)
    with BatchEngine(p, B, precision_mode=MODE) as eng:
        assert eng.precision_mode == MODE
        eng.set_tail_corrections(tail)
        _set(eng, r, v)
        e, d, dd = eng.compute_forces()
        a = _state(eng)[:, 3]
        ek = eng.kinetic_energy()
    for b in range(B):
        em, dm, ddm, am = M.forces(r[b], p.box_length, p.rc, tail=tail)
        assert_bitwise([e[b], d[b], dd[b]], [em, dm, ddm], f"n = {n} replica {b} scalars")
        assert_bitwise(a[b], am, f"n = {n} replica {b} accelerations")
        assert_bitwise(ek[b], M.kinetic(v[b]), f"n = {n} replica {b} ekin")


@pytest.mark.parametrize("n,seeds", [(108, [3, 4, 5]), (500, [3, 4, 5]), (1372, [3, 4, 5]), (4000, [3, 4])])
def test_force_call_bitwise_equals_the_model(n, seeds):
    """one own particle per thread (n = 108, 500), two (1372) and four (4000)"""
    _force_case(n, seeds)


def test_force_call_at_the_largest_cutoff_bitwise_equals_the_model():
    _force_case(500, [6, 7, 8], rc_of_L=(1.0 - 1e-9) * 0.5)


def test_force_call_without_tail_corrections_bitwise_equals_the_model():
    _force_case(500, [3, 4, 5], tail=False)


# ---- 2. a trajectory against the model --------------------------------------------------------------------------------
def test_trajectory_bitwise_equals_the_model():
    g = np.load(GOLDEN / "traj_n108.npz")
    n, B, nsteps = int(g["n"]), 3, 300
    p = init_params(n, float(g["L"]), float(g["dt"]), float(g["rc"]))
    r, v = np.empty((B, 3, n)), np.empty((B, 3, n))
    r[0], v[0] = g["r0"], g["v0"]
    for b, seed in ((1, 91), (2, 92)):
        _, rb, vb = synthetic.make_config(n, seed=seed)
        # the golden run's box, not make_config's: the same lattice scaled into it
        r[b], v[b] = rb * (p.box_length / synthetic.box_length(n)), vb
    with BatchEngine(p, B, precision_mode=MODE) as eng:
        _set(eng, r, v)
        first = eng.compute_forces()
        sc = np.stack(eng.steps(nsteps, sample_every=1), axis=2)             # [nsteps, B, 4]
        st = _state(eng)
    for b in range(B):
        m = M.run(r[b], v[b], p.box_length, p.dt, p.rc, nsteps)
        assert_bitwise([x[b] for x in first], m["first"], f"replica {b} t = 0")
        assert_bitwise(sc[:, b], m["scalars"], f"replica {b} step scalars")
        for k, key in enumerate(("r", "ru", "v", "a")):
            assert_bitwise(st[b, k], m[key], f"replica {b} {key}")


# ---- 3. against the single reproducible engine -----------------------------------------------------------------------
def _engine_run(p, r, v, nsteps):
    with Engine(p, precision_mode=MODE) as eng:
        eng.set_state(r[0], r[1], r[2], v[0], v[1], v[2])
        first = eng.compute_forces()
        sc = np.stack(eng.verlet_steps(nsteps), axis=1)                      # [nsteps, 4]
        st = eng.get_state()
    return first, sc, np.stack([np.stack(st[k]) for k in ("r", "ru", "v", "a")])


def test_equals_the_single_reproducible_engine_n500():
    n, B, nsteps = 500, 2, 50
    p, r, v = _replicas(n, [21, 22])
    with BatchEngine(p, B, precision_mode=MODE) as eng:
        _set(eng, r, v)
        first = eng.compute_forces()
        sc = np.stack(eng.steps(nsteps, sample_every=1), axis=2)
        st = _state(eng)
    for b in range(B):
        f1, sc1, st1 = _engine_run(p, r[b], v[b], nsteps)
        assert_bitwise([x[b] for x in first], f1, f"replica {b} t = 0")
        assert_bitwise(sc[:, b], sc1, f"replica {b} scalars")
        assert_bitwise(st[b], st1, f"replica {b} state")


def test_equals_the_single_reproducible_engine_across_launches_n4000():
    """n = 4000: a launch holds a step or two, so samples every 5 steps fall inside and across launches"""
    n, B, nsteps = 4000, 2, 12
    p, r, v = _replicas(n, [31, 32])
    with BatchEngine(p, B, precision_mode=MODE) as eng:
        _set(eng, r, v)
        first = eng.compute_forces()
        s1 = np.stack(eng.steps(nsteps - 2, sample_every=5), axis=2)         # steps 5, 10
        s2 = np.stack(eng.steps(2, sample_every=2), axis=2)                  # step 12
        assert eng.profile_read()["launches"] >= 1
        st = _state(eng)
    for b in range(B):
        f1, sc1, st1 = _engine_run(p, r[b], v[b], nsteps)
        assert_bitwise([x[b] for x in first], f1, f"replica {b} t = 0")
        assert_bitwise(np.concatenate([s1[:, b], s2[:, b]]), sc1[[4, 9, 11]], f"replica {b} scalars")
        assert_bitwise(st[b], st1, f"replica {b} state")


# ---- 4. independence, bitwise ---------------------------------------------------------------------------------------
def _run(p, r, v, nsteps, sample_every=None):
    with BatchEngine(p, r.shape[0], precision_mode=MODE) as eng:
        _set(eng, r, v)
        f = np.stack(eng.compute_forces(), axis=1)                           # [B, 3]
        sc = eng.steps(nsteps, sample_every or 1, observables=sample_every is not None)
        st = _state(eng)
    return f, None if sc is None else np.stack(sc, axis=2), st


def test_replica_independent_of_batch_size_slot_and_neighbours():
    n, nsteps = 500, 40
    p, mine_r, mine_v = _replicas(n, [77])
    _, other_r, other_v = _replicas(n, range(100, 105))
    alone = _run(p, mine_r, mine_v, nsteps, 10)
    for slot in (0, 4):
        r, v = other_r.copy(), other_v.copy()
        r[slot], v[slot] = mine_r[0], mine_v[0]
        f, sc, st = _run(p, r, v, nsteps, 10)
        assert_bitwise(f[slot], alone[0][0], f"slot {slot} t = 0")
        assert_bitwise(sc[:, slot], alone[1][:, 0], f"slot {slot} scalars")
        assert_bitwise(st[slot], alone[2][0], f"slot {slot} state")
        assert not np.array_equal(st[(slot + 1) % 5], alone[2][0])           # the neighbours did run something else


def test_sampling_interval_changes_no_state():
    n, nsteps = 500, 40
    p, r, v = _replicas(n, [51, 52, 53])
    every, tenth, none = (_run(p, r, v, nsteps, se) for se in (1, 10, None))
    assert none[1] is None
    assert_bitwise(every[2], none[2], "state, sample_every 1 against none")
    assert_bitwise(tenth[2], none[2], "state, sample_every 10 against none")
    assert_bitwise(every[1][9::10], tenth[1], "scalars of steps 10, 20, 30, 40")


MIX = [  # (n, rho, dt, rc_over_L, seed): four kernel classes, each replica with its own L, dt and rc
    (108, 0.80, 0.001, 0.30, 2), (500, 0.95, 0.004, 0.20, 4), (1372, 1.00, 0.002, 0.35, 6), (4000, 0.65, 0.0015, 0.22, 9),
]


def _drive_mix(eng, cfg):
    eng.set_state(*[[c[1][ax] for c in cfg] for ax in range(3)], *[[c[2][ax] for c in cfg] for ax in range(3)])
    f = np.stack(eng.compute_forces(), axis=1)                               # [B, 3]
    k0 = eng.kinetic_energy()
    sc = np.stack(eng.steps(20, 5), axis=2)                                  # [4, B, 4]
    st = eng.get_state()
    state = [[np.asarray(st[key][ax][b]) for key in ("r", "ru", "v", "a") for ax in range(3)] for b in range(len(cfg))]
    return f, k0, sc, state


@pytest.fixture(scope="module")
def mix_reference():
    """the mixed per-replica handle with its groups on streams of their own (the default): computed once"""
    cfg = [synthetic.make_config(n, seed=s, rho=rho, dt=dt, rc_over_L=rcl) for n, rho, dt, rcl, s in MIX]
    with BatchEngine.per_replica([c[0] for c in cfg], precision_mode=MODE) as eng:
        assert eng.precision_mode == MODE
        return cfg, _drive_mix(eng, cfg)


def _same_mix(got, want, b_got, b_want, what):
    for x, y, nm in zip(got[:3], want[:3], ("t = 0", "ekin", "scalars")):
        xs, ys = (x[:, b_got], y[:, b_want]) if nm == "scalars" else (x[b_got], y[b_want])
        assert_bitwise(xs, ys, f"{what} {nm}")
    for x, y in zip(got[3][b_got], want[3][b_want]):
        assert_bitwise(x, y, f"{what} state")


def test_per_replica_handle_equals_one_replica_handles(mix_reference):
    cfg, mixed = mix_reference
    for b, c in enumerate(cfg):
        with BatchEngine(c[0], 1, precision_mode=MODE) as eng:
            eng.set_state(*[c[1][ax][None] for ax in range(3)], *[c[2][ax][None] for ax in range(3)])
            f = np.stack(eng.compute_forces(), axis=1)
            k0 = eng.kinetic_energy()
            sc = np.stack(eng.steps(20, 5), axis=2)
            st = eng.get_state()
        alone = (f, k0, sc, [[st[key][ax][0] for key in ("r", "ru", "v", "a") for ax in range(3)]])
        _same_mix(mixed, alone, b, 0, f"n = {c[0].n}")


def test_group_streams_change_nothing(mix_reference, monkeypatch):
    cfg, mixed = mix_reference
    monkeypatch.setenv("LJMD_BATCH_GROUP_STREAMS", "0")
    with BatchEngine.per_replica([c[0] for c in cfg], precision_mode=MODE) as eng:
        serial = _drive_mix(eng, cfg)
    for b, c in enumerate(cfg):
        _same_mix(serial, mixed, b, b, f"n = {c[0].n}, one stream")


def test_permuted_particles_give_the_permuted_state_and_the_same_scalars():
    """new with this mode: the fp64 batch sums in particle order and does not have this property"""
    n, nsteps = 1372, 20
    p, r, v = _replicas(n, [61, 62])
    perm = np.random.default_rng(7).permutation(n)
    rp, vp = r.copy(), v.copy()
    rp[1], vp[1] = r[1][:, perm], v[1][:, perm]                              # replica 1 permuted, replica 0 as it was
    f, sc, st = _run(p, r, v, nsteps, 5)
    fp, scp, stp = _run(p, rp, vp, nsteps, 5)
    assert_bitwise(fp, f, "t = 0")
    assert_bitwise(scp, sc, "scalars")
    assert_bitwise(stp[0], st[0], "the other replica")
    assert_bitwise(stp[1], st[1][:, :, perm], "permuted state")


# ---- 5. mode switching ------------------------------------------------------------------------------------------------
def test_mode_switching():
    n, B, nsteps = 500, 2, 20
    p, r, v = _replicas(n, [41, 42])
    with BatchEngine(p, B) as eng:
        _set(eng, r, v)
        eng.compute_forces()
        want_sc = np.stack(eng.steps(nsteps, 1), axis=2)
        want_st = _state(eng)
    with BatchEngine(p, B) as eng:
        assert eng.precision_mode == _lib.PRECISION_FP64
        _set(eng, r, v)
        eng.compute_forces()
        eng.set_precision(MODE)
        assert eng.precision_mode == MODE
        for call in (lambda: eng.steps(nsteps, 1), eng.compute_forces):
            with pytest.raises(LjmdError) as ei:
                call()                                                       # the state belonged to the old mode
            assert ei.value.code == _lib.LJMD_ERR_STATE
        for bad in (1, 7):
            with pytest.raises(LjmdError) as ei:
                eng.set_precision(bad)
            assert ei.value.code == _lib.LJMD_ERR_INVALID_ARG
            assert eng.precision_mode == MODE
        _set(eng, r, v)                                                      # ... and the handle keeps working in its mode
        e, d, dd = eng.compute_forces()
        em, dm, ddm, _ = M.forces(r[0], p.box_length, p.rc)
        assert_bitwise([e[0], d[0], dd[0]], [em, dm, ddm], "reproducible after the refused switches")
        eng.steps(3, observables=False)
        eng.set_precision(_lib.PRECISION_FP64)
        with pytest.raises(LjmdError) as ei:
            eng.steps(nsteps, 1)
        assert ei.value.code == _lib.LJMD_ERR_STATE
        _set(eng, r, v)
        eng.compute_forces()
        got_sc = np.stack(eng.steps(nsteps, 1), axis=2)
        got_st = _state(eng)
    assert_bitwise(got_sc, want_sc, "fp64 scalars after 0 -> 2 -> 0")
    assert_bitwise(got_st, want_st, "fp64 state after 0 -> 2 -> 0")


# ---- 6. range -----------------------------------------------------------------------------------------------------------
def test_close_pair_is_a_range_error_naming_the_replica_and_set_state_recovers():
    """an arithmetic flag, not a device fault: the out-of-range terms enter the sums as 0"""
    n, B = 500, 3
    p, r, v = _replicas(n, [71, 72, 73])
    bad = r.copy()
    bad[1, :, 1] = bad[1, :, 0]
    bad[1, 0, 1] += 0.05                               # replica 1: 0.05 sigma apart, u^6 = 0.05^-12 >= 2^40
    with BatchEngine(p, B, precision_mode=MODE) as eng:
        _set(eng, bad, v)
        with pytest.raises(LjmdError) as ei:
            eng.compute_forces()
        assert ei.value.code == _lib.LJMD_ERR_RANGE and "replica 1" in ei.value.message, ei.value.message
        with pytest.raises(LjmdError) as ei:
            eng.steps(1, 1)                            # poisoned
        assert ei.value.code == _lib.LJMD_ERR_STATE
        _set(eng, r, v)
        e, d, dd = eng.compute_forces()
        a = _state(eng)[:, 3]
    for b in range(B):
        em, dm, ddm, am = M.forces(r[b], p.box_length, p.rc)
        assert_bitwise([e[b], d[b], dd[b]], [em, dm, ddm], f"replica {b} after recovery")
        assert_bitwise(a[b], am, f"replica {b} after recovery")


def test_unsampled_step_reports_a_range_error():
    """forces-only steps write no record: the sticky per-replica word carries the flag.  Valid accelerations come from
    set_accel (zeros), so the first thing that meets the 0.05 sigma pair is an unsampled step"""
    n, B = 500, 3
    p, r, v = _replicas(n, [81, 82, 83])
    bad = r.copy()
    bad[2, :, 1] = bad[2, :, 0]
    bad[2, 0, 1] += 0.05                               # replica 2
    zero = np.zeros((B, n))
    with BatchEngine(p, B, precision_mode=MODE) as eng:
        _set(eng, bad, np.zeros_like(v))               # at rest: after the drift the pair is still 0.05 sigma apart
        eng.set_accel(zero, zero, zero)
        with pytest.raises(LjmdError) as ei:
            eng.steps(1, observables=False)
        assert ei.value.code == _lib.LJMD_ERR_RANGE and "replica 2" in ei.value.message, ei.value.message
        with pytest.raises(LjmdError) as ei:
            eng.steps(1, observables=False)            # poisoned
        assert ei.value.code == _lib.LJMD_ERR_STATE
        _set(eng, r, v)
        eng.compute_forces()
        eng.steps(2, observables=False)                # recovered: the flags were cleared
