"""-m gpu: the batch engine (include/ljmd.h, ljmd_batch_*; Python BatchEngine) -- B independent replicas of the same
(n, L, dt, rc) on one device -- against the pinned C oracle, replica by replica, with the single engine's tolerances
(DESIGN.md 3.3), and its determinism: a replica's results do not depend on B, on its slot or on its neighbours, and
the sampling interval changes nothing but which scalars come back."""
import numpy as np
import pytest

from ljmd_amd import BatchEngine, _lib, synthetic
from ljmd_amd._lib import LjmdError

pytestmark = pytest.mark.gpu

REL_SCALAR = 1e-13
REL_ACCEL = 1e-12
REL_TRAJ = 1e-10


def _replicas(n, seeds):
    """-> params, r[B, 3, n], v[B, 3, n]: distinct configurations of the same (n, L, dt, rc)"""
    cfg = [synthetic.make_config(n, seed=s) for s in seeds]
    p = cfg[0][0]
    return p, np.stack([c[1] for c in cfg]), np.stack([c[2] for c in cfg])


def _set(eng, r, v):
    eng.set_state(r[:, 0], r[:, 1], r[:, 2], v[:, 0], v[:, 1], v[:, 2])


def _oracle_state(oracle, po, r, v):
    _, _, _, ax, ay, az = oracle.compute_forces(po, r[0].copy(), r[1].copy(), r[2].copy())
    return {"rx": r[0].copy(), "ry": r[1].copy(), "rz": r[2].copy(),
            "ux": r[0].copy(), "uy": r[1].copy(), "uz": r[2].copy(),
            "vx": v[0].copy(), "vy": v[1].copy(), "vz": v[2].copy(), "ax": ax, "ay": ay, "az": az}


def _series(p, epot, ekin, d_epot):
    etot = epot + ekin
    temp = 2.0 * ekin / (3.0 * p.n)
    press = (p.n / p.volume) * temp + (-d_epot) / (3.0 * p.volume)
    return etot, temp, press


def _rel(a, b):
    return np.abs(a - b) / np.abs(b)


@pytest.mark.parametrize("n", [108, 500, 1372, 4000])
def test_force_parity_per_replica(oracle, n):
    """(a) one force call per replica, B = 5 (n = 1372 and 4000: two and four particles per thread)"""
    p, r, v = _replicas(n, [3, 4, 5, 6, 7])
    po = oracle.derive_params(n, p.box_length, p.dt, p.rc)
    with BatchEngine(p, 5) as eng:
        _set(eng, r, v)
        e, d, dd = eng.compute_forces()
        a = np.stack(eng.get_state(("a",))["a"], axis=1)             # [B, 3, n]
        ek = eng.kinetic_energy()
    for b in range(5):
        e_o, d_o, dd_o, ax, ay, az = oracle.compute_forces(po, r[b, 0].copy(), r[b, 1].copy(), r[b, 2].copy())
        for x, y in ((e[b], e_o), (d[b], d_o), (dd[b], dd_o)):
            assert _rel(x, y) <= REL_SCALAR, (b, x, y)
        ao = np.stack([ax, ay, az])
        assert np.abs(a[b] - ao).max() <= REL_ACCEL * np.abs(ao).max(), b
        ek_o = oracle.ekin_fused(v[b, 0].copy(), v[b, 1].copy(), v[b, 2].copy())
        assert _rel(ek[b], ek_o) <= 1e-13, (b, ek[b], ek_o)


@pytest.mark.parametrize("n", [108, 500])
def test_trajectory_parity_200_steps(oracle, n):
    """(b) Etot, T, P of every step of every replica within 1e-10 of the oracle's run_steps"""
    B, nsteps = 4, 200
    p, r, v = _replicas(n, [21, 22, 23, 24])
    po = oracle.derive_params(n, p.box_length, p.dt, p.rc)
    with BatchEngine(p, B) as eng:
        _set(eng, r, v)
        eng.compute_forces()
        e, k, d, dd = eng.steps(nsteps, sample_every=1)                  # [nsteps, B]
    assert e.shape == (nsteps, B)
    for b in range(B):
        sc = oracle.run_steps(po, nsteps, _oracle_state(oracle, po, r[b], v[b]))
        for nm, x, y in zip(("etot", "T", "P"), _series(p, e[:, b], k[:, b], d[:, b]),
                            _series(p, sc[:, 0], sc[:, 1], sc[:, 2])):
            assert _rel(x, y).max() <= REL_TRAJ, (b, nm, _rel(x, y).max())
        assert _rel(dd[:, b], sc[:, 3]).max() <= REL_TRAJ


def test_steps_across_launches_and_sample_boundaries(oracle):
    """n = 4000: a launch holds a few steps only, so samples every 5 steps fall inside and across launches"""
    n, B, nsteps = 4000, 2, 12
    p, r, v = _replicas(n, [31, 32])
    po = oracle.derive_params(n, p.box_length, p.dt, p.rc)
    with BatchEngine(p, B) as eng:
        _set(eng, r, v)
        eng.compute_forces()
        e, k, d, dd = eng.steps(nsteps - 2, sample_every=5)
        e2, k2, d2, dd2 = eng.steps(2, sample_every=2)
        assert eng.profile_read()["launches"] >= 1
    for b in range(B):
        sc = oracle.run_steps(po, nsteps, _oracle_state(oracle, po, r[b], v[b]))
        got = np.array([[e[0, b], k[0, b], d[0, b], dd[0, b]], [e[1, b], k[1, b], d[1, b], dd[1, b]],
                        [e2[0, b], k2[0, b], d2[0, b], dd2[0, b]]])
        want = sc[[4, 9, 11]]
        assert (np.abs(got - want) / np.abs(want)).max() <= REL_TRAJ, b


def test_integrator_bit_exact_with_the_oracles_accelerations(oracle):
    """(c) set_accel with the oracle's a(t): one step gives r and ru bit for bit"""
    n, B = 500, 3
    p, r, v = _replicas(n, [41, 42, 43])
    po = oracle.derive_params(n, p.box_length, p.dt, p.rc)
    sts = [_oracle_state(oracle, po, r[b], v[b]) for b in range(B)]
    a0 = np.stack([[st["ax"].copy(), st["ay"].copy(), st["az"].copy()] for st in sts])    # [B, 3, n]
    for st in sts:
        oracle.run_steps(po, 1, st)
    with BatchEngine(p, B) as eng:
        _set(eng, r, v)
        eng.set_accel(a0[:, 0], a0[:, 1], a0[:, 2])
        eng.steps(1, observables=False)
        fin = eng.get_state()
    for b, st in enumerate(sts):
        assert np.array_equal(np.stack(fin["r"])[:, b], np.stack([st["rx"], st["ry"], st["rz"]])), b
        assert np.array_equal(np.stack(fin["ru"])[:, b], np.stack([st["ux"], st["uy"], st["uz"]])), b
        assert np.abs(np.stack(fin["v"])[:, b] - np.stack([st["vx"], st["vy"], st["vz"]])).max() < 1e-12


def _run(p, r, v, nsteps, sample_every=None):
    with BatchEngine(p, r.shape[0]) as eng:
        _set(eng, r, v)
        f = eng.compute_forces()
        sc = eng.steps(nsteps, sample_every or 1, observables=sample_every is not None)
        st = eng.get_state()
    return f, sc, np.stack([np.stack(st[k], axis=1) for k in ("r", "ru", "v", "a")], axis=1)   # [B, 4, 3, n]


def test_replica_independent_of_batch_size_slot_and_neighbours():
    """(d) the same replica alone, at slot 0 and at slot 37 of B = 64 beside other replicas: bitwise equal, and
    bitwise equal run to run"""
    n, nsteps = 500, 100
    p, mine_r, mine_v = _replicas(n, [77])
    _, other_r, other_v = _replicas(n, range(100, 164))
    alone = _run(p, mine_r, mine_v, nsteps, 10)
    again = _run(p, mine_r, mine_v, nsteps, 10)
    for slot in (0, 37):
        r, v = other_r.copy(), other_v.copy()
        r[slot], v[slot] = mine_r[0], mine_v[0]
        f, sc, st = _run(p, r, v, nsteps, 10)
        assert np.array_equal(st[slot], alone[2][0]), slot
        for x, y in zip(f, alone[0]):
            assert x[slot] == y[0], slot
        for x, y in zip(sc, alone[1]):
            assert np.array_equal(x[:, slot], y[:, 0]), slot
        assert not np.array_equal(st[(slot + 1) % 64], alone[2][0])       # the neighbours did run something else
    assert np.array_equal(again[2], alone[2])
    assert all(np.array_equal(x, y) for x, y in zip(again[1], alone[1]))


def test_sampling_interval_changes_no_state():
    """(e) 100 steps with sample_every 1, 10, 100 and without outputs: identical r, ru, v, a; identical scalars of
    step 100"""
    n, nsteps = 500, 100
    p, r, v = _replicas(n, [51, 52, 53])
    runs = {se: _run(p, r, v, nsteps, se) for se in (1, 10, 100, None)}
    ref = runs[None][2]
    for se in (1, 10, 100):
        assert np.array_equal(runs[se][2], ref), se
        last = [x[-1] for x in runs[se][1]]
        assert all(np.array_equal(x, y) for x, y in zip(last, [x[-1] for x in runs[100][1]])), se
        assert runs[se][1][0].shape == (nsteps // se, 3)
    assert runs[None][1] is None


def test_tail_corrections_switch_off_vs_oracle(oracle):
    """(f) without the tail constants the scalars match the oracle's else-branch; forces and ekin do not change"""
    n, B = 500, 3
    p, r, v = _replicas(n, [61, 62, 63])
    po = oracle.derive_params(n, p.box_length, p.dt, p.rc)
    oracle.set_tail_corrections(False)
    try:
        off = [oracle.compute_forces(po, r[b, 0].copy(), r[b, 1].copy(), r[b, 2].copy()) for b in range(B)]
        sc_off = [oracle.run_steps(po, 5, _oracle_state(oracle, po, r[b], v[b])) for b in range(B)]
    finally:
        oracle.set_tail_corrections(True)
    te = oracle.tail_corrections(po)
    with BatchEngine(p, B) as eng:
        _set(eng, r, v)
        on = eng.compute_forces()
        a_on = np.stack(eng.get_state(("a",))["a"])
        eng.set_tail_corrections(False)
        f = eng.compute_forces()
        a_off = np.stack(eng.get_state(("a",))["a"])
        steps = eng.steps(5, 1)
    assert np.array_equal(a_on, a_off)
    for b in range(B):
        for k in range(3):
            assert _rel(f[k][b], off[b][k]) <= REL_SCALAR, (b, k)
            assert abs(on[k][b] - f[k][b] - te[k]) <= 1e-9 * abs(te[k]), (b, k)
        for col in range(4):
            assert (_rel(steps[col][:, b], sc_off[b][:, col])).max() <= REL_TRAJ, (b, col)


def test_sequence_errors_and_guards():
    """(g) steps before set_state or before forces: LJMD_ERR_STATE; a replica spanning >= 2.4 L: LJMD_ERR_INVALID_ARG"""
    n, B = 108, 2
    p, r, v = _replicas(n, [1, 2])
    with BatchEngine(p, B) as eng:
        for call in (lambda: eng.steps(10, 1), lambda: eng.steps(10, observables=False), eng.compute_forces,
                     eng.kinetic_energy, eng.get_state):
            with pytest.raises(LjmdError) as ei:
                call()
            assert ei.value.code == _lib.LJMD_ERR_STATE
        with pytest.raises(LjmdError) as ei:
            eng.set_accel(r[:, 0], r[:, 1], r[:, 2])
        assert ei.value.code == _lib.LJMD_ERR_STATE
        _set(eng, r, v)
        with pytest.raises(LjmdError) as ei:
            eng.steps(10, 1)                                              # no accelerations yet
        assert ei.value.code == _lib.LJMD_ERR_STATE and "accelerations" in ei.value.message
        with pytest.raises(LjmdError) as ei:
            eng.set_accel(None, None, None)                               # nothing valid to keep yet
        assert ei.value.code == _lib.LJMD_ERR_INVALID_ARG
        with pytest.raises(LjmdError) as ei:
            eng.set_accel(r[:, 0], None, r[:, 2])
        assert ei.value.code == _lib.LJMD_ERR_INVALID_ARG
        with pytest.raises(LjmdError) as ei:
            eng.steps(10, 1)                                              # still no accelerations
        assert ei.value.code == _lib.LJMD_ERR_STATE
        bad = r.copy()
        bad[1, 2, 5] += 3.0 * p.box_length                               # replica 1 spans > 2.4 L along z
        with pytest.raises(LjmdError) as ei:
            eng.set_state(bad[:, 0], bad[:, 1], bad[:, 2], v[:, 0], v[:, 1], v[:, 2])
        assert ei.value.code == _lib.LJMD_ERR_INVALID_ARG and "2.4 L" in ei.value.message
        bad[1, 2, 5] = np.nan
        with pytest.raises(LjmdError) as ei:
            eng.set_state(bad[:, 0], bad[:, 1], bad[:, 2], v[:, 0], v[:, 1], v[:, 2])
        assert ei.value.code == _lib.LJMD_ERR_INVALID_ARG
        with pytest.raises(LjmdError) as ei:
            eng.steps(10, 1)                                              # the failed set_state changed nothing
        assert ei.value.code == _lib.LJMD_ERR_STATE
        eng.compute_forces()
        lib = _lib.load()
        assert lib.ljmd_batch_steps(eng._h, 10, 3, None, None, None, None) == _lib.LJMD_OK   # nothing sampled
        out = np.empty(8)
        assert lib.ljmd_batch_steps(eng._h, 10, 3, out.ctypes.data_as(_lib.c_double_p), None, None, None) \
            == _lib.LJMD_ERR_INVALID_ARG                                 # 10 % 3
        assert lib.ljmd_batch_steps(eng._h, -1, 1, None, None, None, None) == _lib.LJMD_ERR_INVALID_ARG
        big = np.empty(2 * 4097)
        assert lib.ljmd_batch_steps(eng._h, 4097, 1, big.ctypes.data_as(_lib.c_double_p), None, None, None) \
            == _lib.LJMD_ERR_INVALID_ARG                                 # > LJMD_MAX_PENDING_STEPS samples
        e, k, d, dd = eng.steps(10, 5)
        assert e.shape == (2, B) and np.all(np.isfinite(e)) and np.all(k > 0)
        a = eng.get_state(("a",))["a"]
        eng.set_accel(None, a[1] * 2.0, None)                            # valid accelerations: NULL keeps a component
        a2 = eng.get_state(("a",))["a"]
        assert np.array_equal(a2[0], a[0]) and np.array_equal(a2[1], a[1] * 2.0) and np.array_equal(a2[2], a[2])
    with pytest.raises(LjmdError) as ei:
        BatchEngine(p, 2, device=1 << 20)
    assert ei.value.code == _lib.LJMD_ERR_INVALID_ARG
