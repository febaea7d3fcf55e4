"""-m gpu: batch handles whose replicas each have their own (n, L, dt, rc) (ljmd_batch_create_per_replica; Python
PerReplicaBatchEngine).  The contract: a replica's r, ru, v, a and scalars are bitwise those of a one-replica
ljmd_batch_create handle of the same replica, whatever the other replicas, their order, B, the launch grouping or
the chunking; against the oracle they meet the tolerances of the homogeneous engine (tests/test_gpu_batch.py)."""
import numpy as np
import pytest

from ljmd_amd import BatchEngine, _lib, synthetic
from ljmd_amd._lib import LjmdError

pytestmark = pytest.mark.gpu

REL_SCALAR = 1e-13
REL_ACCEL = 1e-12
REL_TRAJ = 1e-10

# all five kernel classes (<= 128, 512, 1024, 2048, 4096), densities 0.5 .. 1.0, dt 1e-4 .. 5e-3, rc/L 0.2 .. 0.49
MIX = [  # (n, rho, dt, rc_over_L, seed)
    (32, 0.60, 0.005, 0.49, 1), (108, 0.80, 0.001, 0.30, 2), (256, 0.50, 0.0005, 0.45, 3),
    (500, 0.95, 0.004, 0.20, 4), (864, 0.70, 0.0001, 0.40, 5), (1372, 1.00, 0.002, 0.35, 6),
    (2048, 0.55, 0.003, 0.25, 7), (2916, 0.85, 0.0025, 0.49, 8), (4000, 0.65, 0.0015, 0.22, 9),
    (100, 0.90, 0.0035, 0.49, 10), (700, 0.75, 0.0045, 0.33, 11), (1500, 0.60, 0.005, 0.28, 12),
]


def _configs(spec):
    return [synthetic.make_config(n, seed=s, rho=rho, dt=dt, rc_over_L=rcl) for n, rho, dt, rcl, s in spec]


def _drive(eng, cfg):
    """set_state, compute_forces, then steps with and without sampling, long enough that the largest replicas need
    several launches per call -> (forces scalars, list of step scalars, state per replica)"""
    eng.set_state(*[[c[1][ax] for c in cfg] for ax in range(3)], *[[c[2][ax] for c in cfg] for ax in range(3)])
    f = eng.compute_forces()
    k0 = eng.kinetic_energy()
    s1 = eng.steps(30, 5)
    eng.steps(13, observables=False)
    s2 = eng.steps(12, 12)
    st = eng.get_state()
    return f, k0, (s1, s2), st


def _replica(res, b):
    f, k0, (s1, s2), st = res
    scal = [x[b] for x in f] + [k0[b]] + [x[:, b] for x in s1] + [x[:, b] for x in s2]
    state = [st[key][ax][b] if isinstance(st[key][ax], list) else st[key][ax][0]
             for key in ("r", "ru", "v", "a") for ax in range(3)]
    return scal, state


def _single(c):
    p, r, v = c
    with BatchEngine(p, 1) as eng:
        res = _drive(eng, [c])
    f, k0, ss, st = res
    st = {k: tuple([x[0]] for x in st[k]) for k in st}
    return _replica((f, k0, ss, st), 0)


def _equal(x, y):
    return all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(x, y))


def test_replicas_bitwise_independent_of_neighbours_order_and_grouping():
    cfg = _configs(MIX)
    B = len(cfg)
    with BatchEngine.per_replica([c[0] for c in cfg]) as eng:
        assert list(eng.offsets) == list(np.concatenate([[0], np.cumsum([c[0].n for c in cfg])]))
        fwd = _drive(eng, cfg)
        prof = eng.profile_read()
        assert prof["launches"] > 5, prof           # five groups, the large ones split into several launches
    rev_cfg = cfg[::-1]
    with BatchEngine.per_replica([c[0] for c in rev_cfg]) as eng:
        rev = _drive(eng, rev_cfg)
    for b, c in enumerate(cfg):
        alone = _single(c)
        mine = _replica(fwd, b)
        assert _equal(mine[1], alone[1]), (b, c[0].n)
        assert _equal(mine[0], alone[0]), (b, c[0].n)
        back = _replica(rev, B - 1 - b)
        assert _equal(back[1], alone[1]) and _equal(back[0], alone[0]), (b, c[0].n)
        assert np.isfinite(mine[0][4]).all()


def test_equal_parameters_match_the_homogeneous_handle_bitwise():
    """B = 300 at n = 108: one group, chunked launches; the same bits as ljmd_batch_create"""
    B, n = 300, 108
    cfg = [synthetic.make_config(n, seed=500 + b) for b in range(B)]
    p = cfg[0][0]
    with BatchEngine.per_replica([p] * B) as eng:
        per = _drive(eng, cfg)
    with BatchEngine(p, B) as eng:
        r = np.stack([c[1] for c in cfg])
        v = np.stack([c[2] for c in cfg])
        eng.set_state(r[:, 0], r[:, 1], r[:, 2], v[:, 0], v[:, 1], v[:, 2])
        f = eng.compute_forces()
        k0 = eng.kinetic_energy()
        s1 = eng.steps(30, 5)
        eng.steps(13, observables=False)
        s2 = eng.steps(12, 12)
        st = eng.get_state()
    assert _equal(per[0], f) and np.array_equal(per[1], k0)
    assert _equal(per[2][0], s1) and _equal(per[2][1], s2)
    for key in ("r", "ru", "v", "a"):
        for ax in range(3):
            assert np.array_equal(np.stack(per[3][key][ax]), st[key][ax]), key


def _oracle_state(oracle, po, r, v):
    _, _, _, ax, ay, az = oracle.compute_forces(po, r[0].copy(), r[1].copy(), r[2].copy())
    return {"rx": r[0].copy(), "ry": r[1].copy(), "rz": r[2].copy(),
            "ux": r[0].copy(), "uy": r[1].copy(), "uz": r[2].copy(),
            "vx": v[0].copy(), "vy": v[1].copy(), "vz": v[2].copy(), "ax": ax, "ay": ay, "az": az}


def _rel(a, b):
    return np.abs(a - b) / np.abs(b)


def test_oracle_parity_per_replica(oracle):
    """forces and t = 0 scalars of every replica of the mix; 200-step series of the small ones"""
    cfg = _configs(MIX)
    with BatchEngine.per_replica([c[0] for c in cfg]) as eng:
        eng.set_state(*[[c[1][ax] for c in cfg] for ax in range(3)], *[[c[2][ax] for c in cfg] for ax in range(3)])
        e, d, dd = eng.compute_forces()
        a = eng.get_state(("a",))["a"]
        ek = eng.kinetic_energy()
    for b, (p, r, v) in enumerate(cfg):
        po = oracle.derive_params(p.n, p.box_length, p.dt, p.rc)
        e_o, d_o, dd_o, ax, ay, az = oracle.compute_forces(po, r[0].copy(), r[1].copy(), r[2].copy())
        for x, y in ((e[b], e_o), (d[b], d_o), (dd[b], dd_o)):
            assert _rel(x, y) <= REL_SCALAR, (b, x, y)
        ao = np.stack([ax, ay, az])
        assert np.abs(np.stack([a[k][b] for k in range(3)]) - ao).max() <= REL_ACCEL * np.abs(ao).max(), b
        assert _rel(ek[b], oracle.ekin_fused(v[0].copy(), v[1].copy(), v[2].copy())) <= 1e-13, b

    small = _configs([s for s in MIX if s[0] <= 500])
    nsteps = 200
    with BatchEngine.per_replica([c[0] for c in small]) as eng:
        eng.set_state(*[[c[1][ax] for c in small] for ax in range(3)],
                      *[[c[2][ax] for c in small] for ax in range(3)])
        eng.compute_forces()
        e, k, d, dd = eng.steps(nsteps, 1)
    for b, (p, r, v) in enumerate(small):
        po = oracle.derive_params(p.n, p.box_length, p.dt, p.rc)
        sc = oracle.run_steps(po, nsteps, _oracle_state(oracle, po, r, v))
        etot, etot_o = e[:, b] + k[:, b], sc[:, 0] + sc[:, 1]
        temp, temp_o = 2.0 * k[:, b] / (3.0 * p.n), 2.0 * sc[:, 1] / (3.0 * p.n)
        press = (p.n / p.volume) * temp - d[:, b] / (3.0 * p.volume)
        press_o = (p.n / p.volume) * temp_o - sc[:, 2] / (3.0 * p.volume)
        for nm, x, y in (("etot", etot, etot_o), ("T", temp, temp_o), ("P", press, press_o), ("dd", dd[:, b], sc[:, 3])):
            assert _rel(x, y).max() <= REL_TRAJ, (b, nm, _rel(x, y).max())


def test_tail_corrections_are_each_replicas_own(oracle):
    cfg = _configs(MIX[:6])
    with BatchEngine.per_replica([c[0] for c in cfg]) as eng:
        eng.set_state(*[[c[1][ax] for c in cfg] for ax in range(3)], *[[c[2][ax] for c in cfg] for ax in range(3)])
        on = eng.compute_forces()
        eng.set_tail_corrections(False)
        off = eng.compute_forces()
    for b, (p, _, _) in enumerate(cfg):
        te = oracle.tail_corrections(oracle.derive_params(p.n, p.box_length, p.dt, p.rc))
        for k in range(3):
            assert abs(on[k][b] - off[k][b] - te[k]) <= 1e-9 * abs(te[k]), (b, k)


def test_sequence_errors_and_per_replica_span_guard():
    cfg = _configs(MIX[:3])
    r = [[c[1][ax] for c in cfg] for ax in range(3)]
    v = [[c[2][ax] for c in cfg] for ax in range(3)]
    with BatchEngine.per_replica([c[0] for c in cfg]) as eng:
        for call in (lambda: eng.steps(10, 1), lambda: eng.steps(10, observables=False), eng.compute_forces,
                     eng.kinetic_energy, eng.get_state):
            with pytest.raises(LjmdError) as ei:
                call()
            assert ei.value.code == _lib.LJMD_ERR_STATE
        eng.set_state(*r, *v)
        with pytest.raises(LjmdError) as ei:
            eng.steps(10, 1)
        assert ei.value.code == _lib.LJMD_ERR_STATE and "accelerations" in ei.value.message
        # replica 0 (the smallest box) spread over 2.4 of its own L: rejected, though it fits the other boxes
        L0 = cfg[0][0].box_length
        bad = [x.copy() for x in r[0]]
        bad[0][0] = bad[0][1] + 2.5 * L0
        assert 2.5 * L0 < 2.4 * cfg[2][0].box_length
        with pytest.raises(LjmdError) as ei:
            eng.set_state(bad, r[1], r[2], *v)
        assert ei.value.code == _lib.LJMD_ERR_INVALID_ARG and "replica 0" in ei.value.message
        eng.set_state(*r, *v)
        eng.compute_forces()
        eng.steps(10, 5)
