"""-m gpu: the reproducible mode (LJMD_PRECISION_FP64_REPRODUCIBLE).  Its results are a function of the particle set
alone: bitwise equal to the CPU model of the definition (tests/reproducible_model.py) and bitwise independent of input
order, rank count, re-sorting and launch form; against the reference they keep the fp64 mode's bounds."""
import numpy as np
import pytest

import ljmd_amd
import reproducible_model as M
from ljmd_amd import Engine, _lib, init_params, synthetic
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


def gpu_force(p, r, v=None, **kw):
    with Engine(p, precision_mode=MODE, **kw) as eng:
        v = np.zeros_like(r) if v is None else v
        eng.set_state(r[0], r[1], r[2], v[0], v[1], v[2])
        assert eng.pair_kernel_name() == "pair_fixed_kernel"
        sc = eng.compute_forces()
        a = np.stack(eng.get_state(("a",))["a"])
        k = eng.kinetic_energy()
    return sc, a, k


def force_inputs():
    out = []
    g = np.load(GOLDEN / "force_fcc108.npz")
    L = float(g["L"])
    from oracle import oracle as O
    rx, ry, rz = O.fcc_lattice(3, L)
    out.append(("fcc108", init_params(108, L, 0.005, float(g["rc"]), num_cells=3), np.stack([rx, ry, rz]), None))
    for n in (500, 4096):
        p, r, v = synthetic.make_config(n)
        out.append((f"jitter{n}", p, r, v))
    p, r, v = synthetic.make_config(4096)
    out.append(("rc0.1L", init_params(4096, p.box_length, p.dt, 0.1 * p.box_length), r, v))
    g = np.load(GOLDEN / "force_n500_unwrapped.npz")
    out.append(("unwrapped", init_params(500, float(g["L"]), 0.005, float(g["rc"])), np.array(g["r"]), None))
    p, r, v = synthetic.make_config(500)
    out.append(("rc_half_box", init_params(500, p.box_length, p.dt, 0.5 * p.box_length * (1.0 - 1e-10)), r, v))
    return out


@pytest.mark.parametrize("case", force_inputs(), ids=lambda c: c[0])
def test_force_call_bitwise_equals_the_model(case):
    name, p, r, v = case
    (e, d, dd), a, k = gpu_force(p, r, v)
    em, dm, ddm, am = M.forces(r, p.box_length, p.rc)
    assert_bitwise([e, d, dd], [em, dm, ddm], name + " scalars")
    assert_bitwise(a, am, name + " accelerations")
    if v is not None:
        assert_bitwise(k, M.kinetic(v), name + " ekin")


@pytest.mark.parametrize("name,nsteps", [("traj_n108", 1000), ("traj_n4096_200", 10)])
def test_trajectory_bitwise_equals_the_model(golden, name, nsteps):
    g = golden(name)
    n = int(g["n"])
    p = init_params(n, float(g["L"]), float(g["dt"]), float(g["rc"]))
    r0, v0 = g["r0"], g["v0"]
    with Engine(p, precision_mode=MODE) as eng:
        eng.set_state(r0[0], r0[1], r0[2], v0[0], v0[1], v0[2])
        first = eng.compute_forces()
        sc = np.stack(eng.verlet_steps(nsteps), axis=1)
        st = eng.get_state()
    m = M.run(r0, v0, p.box_length, p.dt, p.rc, nsteps)
    assert_bitwise(first, m["first"], "t = 0")
    assert_bitwise(sc, m["scalars"], "step scalars")
    for key in ("r", "ru", "v", "a"):
        assert_bitwise(np.stack(st[key]), m[key], key)


# ---- invariances, bitwise, GPU against GPU --------------------------------------------------------------------------
N_INV, STEPS_INV = 16384, 200


def _run(p, r, v, nsteps, sampled=False, **kw):
    with Engine(p, precision_mode=MODE, **kw) as eng:
        eng.set_state(r[0], r[1], r[2], v[0], v[1], v[2])
        first = eng.compute_forces()
        if sampled:
            eng.enqueue_steps(nsteps, sampled=True)
            sc = np.stack(eng.collect_steps(nsteps), axis=1)
        else:
            sc = np.stack(eng.verlet_steps(nsteps), axis=1)
        st = eng.get_state()
    return first, sc, {k: np.stack(st[k]) for k in ("r", "ru", "v", "a")}


@pytest.fixture(scope="module")
def inv_reference():
    p, r, v = synthetic.make_config(N_INV, seed=11)
    return p, r, v, _run(p, r, v, STEPS_INV)


def _same(ref, got, what, perm=None):
    first, sc, st = ref
    first2, sc2, st2 = got
    assert_bitwise(first, first2, what + " t = 0")
    assert_bitwise(sc, sc2, what + " scalars")
    for k in st:
        assert_bitwise(st[k] if perm is None else st[k][:, perm], st2[k], what + " " + k)


def test_permuted_input_gives_the_permuted_output(inv_reference):
    p, r, v, ref = inv_reference
    perm = np.random.default_rng(7).permutation(p.n)
    _same(ref, _run(p, np.ascontiguousarray(r[:, perm]), np.ascontiguousarray(v[:, perm]), STEPS_INV), "permuted", perm)


@pytest.mark.parametrize("G", [1, 2, 4, 8])
def test_rank_count_one_card(inv_reference, G):
    p, r, v, ref = inv_reference
    _same(ref, _run(p, r, v, STEPS_INV, devices=[0] * G), f"G = {G}")


@pytest.mark.parametrize("env", [{"LJMD_RESORT_EVERY": "1"}, {"LJMD_RESORT_EVERY": "1000"}, {"LJMD_SORT": "0"},
                                 {"LJMD_FUSE": "0"}])
def test_resort_and_launch_knobs(inv_reference, env, monkeypatch):
    p, r, v, ref = inv_reference
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    _same(ref, _run(p, r, v, STEPS_INV), str(env))


def test_sampled_segments_equal_verlet_steps(inv_reference):
    p, r, v, ref = inv_reference
    first, sc, st = _run(p, r, v, STEPS_INV, sampled=True)
    assert np.isnan(sc[:-1, 0]).all() and np.isnan(sc[:-1, 2]).all()
    assert_bitwise(sc[-1], ref[1][-1], "sampled last step")
    assert_bitwise(sc[:, 1], ref[1][:, 1], "ekin")
    for k in st:
        assert_bitwise(ref[2][k], st[k], "sampled " + k)


def _hip():
    import ctypes as C
    hip = C.CDLL("libamdhip64.so.7")       # already loaded by libljmd.so: same runtime instance
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMemcpy.restype = C.c_int
    return hip


def _allgather(engines):
    hip = _hip()
    for e in engines:
        e.synchronize()
    for src in engines:
        sp, _tot, off, cnt = src.exchange_buffer()
        for dst in engines:
            if dst is not src:
                assert hip.hipMemcpy(dst.exchange_buffer()[0] + 8 * off, sp + 8 * off, 8 * cnt, 3) == 0
    assert hip.hipDeviceSynchronize() == 0


def test_two_split_phase_ranks_host_staged(inv_reference):
    """The one-process-per-GPU form: every rank owns its rows completely (no force exchange); the exact records are
    combined as integers (ljmd_read_partials_exact / ljmd_combine_scalars_exact)."""
    p, r, v, ref = inv_reference
    nsteps, G = 50, 2
    engines = [Engine(p, rank=g, n_ranks=G, precision_mode=MODE) for g in range(G)]
    try:
        for e in engines:
            e.set_state(r[0], r[1], r[2], v[0], v[1], v[2])
        _allgather(engines)
        for e in engines:
            e.forces_partial()
        with pytest.raises(ljmd_amd.LjmdError):
            engines[0].read_partials(1)                  # the double records do not exist in this mode
        w0 = np.stack([e.read_partials_exact(1)[0] for e in engines])
        t0 = engines[0].combine_scalars_exact(w0)
        assert_bitwise([t0[0], t0[2], t0[3]], ref[0], "t = 0")
        for _ in range(nsteps):
            for e in engines:
                e.step_begin()
            _allgather(engines)
            for e in engines:
                e.step_finish()
        w = np.stack([e.read_partials_exact(nsteps) for e in engines])
        sc = np.array([engines[0].combine_scalars_exact(np.ascontiguousarray(w[:, s])) for s in range(nsteps)])
        S = p.n // G
        st = {k: np.concatenate([np.stack(e.get_state((k,))[k]) for e in engines], axis=1) for k in ("r", "v", "a")}
    finally:
        for e in engines:
            e.close()
    with Engine(p, precision_mode=MODE) as one:
        one.set_state(r[0], r[1], r[2], v[0], v[1], v[2])
        one.compute_forces()
        sc1 = np.stack(one.verlet_steps(nsteps), axis=1)
        st1 = one.get_state(("r", "v", "a"))
    assert_bitwise(sc, sc1, "split-phase scalars")
    for k in st:
        assert st[k].shape[1] == G * S
        assert_bitwise(st[k], np.stack(st1[k]), "split-phase " + k)


def test_stateless_drop_ins_equal_an_engine(monkeypatch):
    from ljmd_amd import init_state
    from ljmd_amd.physics import stateless_reset
    monkeypatch.setenv("LJMD_REPRODUCIBLE", "1")
    stateless_reset()
    try:
        p, r, v = synthetic.make_config(4096, seed=3)
        st = init_state(p)
        st.rx[:], st.ry[:], st.rz[:] = r
        st.vx[:], st.vy[:], st.vz[:] = v
        first = ljmd_amd.compute_lj_potential_energy(p, st)
        sc = [ljmd_amd.verlet_step(p, st) for _ in range(20)]
    finally:
        stateless_reset()
    ref_first, ref_sc, ref_st = _run(p, r, v, 20)
    assert_bitwise(first, ref_first, "stateless t = 0")
    assert_bitwise(np.array(sc), ref_sc, "stateless scalars")
    assert_bitwise(np.stack([st.rx, st.ry, st.rz]), ref_st["r"], "stateless r")
    assert_bitwise(np.stack([st.vx, st.vy, st.vz]), ref_st["v"], "stateless v")
    assert_bitwise(np.stack([st.ax, st.ay, st.az]), ref_st["a"], "stateless a")


def test_one_force_call_n262144_permutation_and_ranks():
    p, r, v = synthetic.make_config(262144, seed=2)
    (e, d, dd), a, k = gpu_force(p, r, v)
    perm = np.random.default_rng(9).permutation(p.n)
    (e2, d2, dd2), a2, k2 = gpu_force(p, np.ascontiguousarray(r[:, perm]), np.ascontiguousarray(v[:, perm]))
    assert_bitwise([e, d, dd, k], [e2, d2, dd2, k2], "permuted scalars")
    assert_bitwise(a[:, perm], a2, "permuted accelerations")
    (e4, d4, dd4), a4, k4 = gpu_force(p, r, v, devices=[0] * 4)
    assert_bitwise([e, d, dd, k], [e4, d4, dd4, k4], "G = 4 scalars")
    assert_bitwise(a, a4, "G = 4 accelerations")


# ---- against the reference, at the fp64 mode's bounds ---------------------------------------------------------------
@pytest.mark.parametrize("name", ["force_n108", "force_n500", "force_n4000", "force_n4096", "force_n500_unwrapped"])
def test_force_call_vs_reference_golden(golden, name):
    g = golden(name)
    n = int(g["n"])
    p = init_params(n, float(g["L"]), 0.005, float(g["rc"]))
    (e, d, dd), a, _k = gpu_force(p, np.array(g["r"]))
    for x, y in zip((e, d, dd), g["scalars"]):
        assert abs(x - y) <= 1e-13 * abs(y), (name, x, y)
    amax = np.max(np.abs(g["a"]))
    assert np.max(np.abs(a - g["a"])) <= 1e-12 * max(amax, 1.0)


@pytest.mark.parametrize("name", ["traj_n108", "traj_n4096_200"])
def test_short_trajectory_vs_reference_golden(golden, name):
    g = golden(name)
    n = int(g["n"])
    p = init_params(n, float(g["L"]), float(g["dt"]), float(g["rc"]))
    r0, v0 = g["r0"], g["v0"]
    with Engine(p, precision_mode=MODE) as eng:
        eng.set_state(r0[0], r0[1], r0[2], v0[0], v0[1], v0[2])
        e, d, dd = eng.compute_forces()
        s0 = (e, eng.kinetic_energy(), d, dd)
        mine = np.vstack([s0, np.stack(eng.verlet_steps(200), axis=1)])
    ref = g["scalars"][:201]

    def series(sc):
        temp = 2.0 * sc[:, 1] / (3.0 * p.n)
        return sc[:, 0] + sc[:, 1], temp, (p.n / p.volume) * temp + (-sc[:, 2]) / (3.0 * p.volume)

    for nm, x, y in zip(("etot", "T", "P"), series(mine), series(ref)):
        assert np.max(np.abs(x - y) / np.abs(y)) <= 1e-10, (name, nm)


def test_liquid_state_forces_vs_oracle_n65536(oracle):
    n = 65536
    p, r, v = synthetic.make_config(n, seed=23)
    with Engine(p, precision_mode=MODE) as eng:
        eng.set_state(r[0], r[1], r[2], v[0], v[1], v[2])
        eng.compute_forces()
        eng.enqueue_steps(100, sampled=True)
        e, _k, d, dd = eng.collect_steps(100)
        rr = np.stack(eng.get_state(("r",))["r"])
        a = np.stack(eng.get_state(("a",))["a"])
    po = oracle.derive_params(n, p.box_length, p.dt, p.rc)
    e_o, d_o, dd_o, ax, ay, az = oracle.compute_forces(po, rr[0].copy(), rr[1].copy(), rr[2].copy())
    a_o = np.stack([ax, ay, az])
    for x, y in ((e[-1], e_o), (d[-1], d_o), (dd[-1], dd_o)):
        assert abs(x - y) <= 1e-12 * abs(y), (x, y)
    assert np.abs(a - a_o).max() <= 1e-12 * np.abs(a_o).max()


# ---- range ----------------------------------------------------------------------------------------------------------
def test_close_pair_is_a_range_error_and_set_state_recovers():
    p, r, v = synthetic.make_config(500)
    bad = r.copy()
    bad[:, 1] = bad[:, 0]
    bad[0, 1] += 0.05                                  # 0.05 sigma apart: u^6 = 0.05^-12 >= 2^40
    with Engine(p, precision_mode=MODE) as eng:
        eng.set_state(bad[0], bad[1], bad[2], v[0], v[1], v[2])
        with pytest.raises(ljmd_amd.LjmdError) as ei:
            eng.compute_forces()
        assert ei.value.code == _lib.LJMD_ERR_RANGE
        with pytest.raises(ljmd_amd.LjmdError) as ei:
            eng.verlet_steps(1)                        # poisoned
        assert ei.value.code == _lib.LJMD_ERR_STATE
        eng.set_state(r[0], r[1], r[2], v[0], v[1], v[2])
        sc = eng.compute_forces()
        a = np.stack(eng.get_state(("a",))["a"])
    em, dm, ddm, am = M.forces(r, p.box_length, p.rc)
    assert_bitwise(sc, [em, dm, ddm], "after recovery")
    assert_bitwise(a, am, "after recovery")


def test_create_refuses_what_the_mode_cannot_hold():
    p = init_params(1 << 24, 300.0, 0.005, 2.5)
    with pytest.raises(ljmd_amd.LjmdError) as ei:
        Engine(p, precision_mode=MODE)
    assert ei.value.code == _lib.LJMD_ERR_INVALID_ARG


# ---- Fortran driver -------------------------------------------------------------------------------------------------
def _fortran_run(tmp_path, tag, env_extra):
    import os
    import shutil
    import subprocess
    from conftest import ROOT
    exe = ROOT / "molecular-dynamics-simulation---lennard-jones-monoatomic-fluid_amd" / "bin" / "md_simulation_gpu"
    src = GOLDEN / "ref_run_n108_oi100"
    d = tmp_path / tag
    (d / "inputs").mkdir(parents=True)
    (d / "outputs" / "one_run").mkdir(parents=True)
    shutil.copy(src / "input_simulation_parameters.txt", d / "inputs")
    shutil.copy(src / "rv_init.dat", d / "outputs")
    env = dict(os.environ, LJMD_REPRODUCIBLE="1", **env_extra)
    subprocess.run([str(exe)], cwd=d, env=env, check=True, timeout=300, capture_output=True)
    return {f.name: f.read_bytes() for f in sorted((d / "outputs" / "one_run").iterdir()) if f.is_file()}


def test_fortran_driver_output_files_independent_of_gpu_count(tmp_path):
    one = _fortran_run(tmp_path, "g1", {"LJMD_GPUS": "1"})
    four = _fortran_run(tmp_path, "g4", {"LJMD_GPUS": "4", "LJMD_DEVICES": "0,0,0,0"})
    assert "rva.dat" in one and "instantaneous_energies.dat" in one
    assert sorted(one) == sorted(four)
    for name in one:
        assert one[name] == four[name], name


def test_distributed_layer_combines_the_exact_records():
    """distributed.ShardedSimulation (bench.py's one-process-per-GPU layer) reads ljmd_read_partials_exact and combines with
    ljmd_combine_scalars_exact on a reproducible engine: the same bits as the engine's own verlet_steps."""
    from ljmd_amd import distributed
    p, r, v = synthetic.make_config(4096, seed=13)
    with Engine(p, precision_mode=MODE) as eng:
        distributed.bootstrap_rccl(eng, 0, 1)
        sim = distributed.ShardedSimulation(eng, 0, 1)
        first = sim.start(r, v)
        sc = np.stack(sim.run(10), axis=1)
    ref_first, ref_sc, _st = _run(p, r, v, 10)
    assert_bitwise(first, ref_first, "distributed t = 0")
    assert_bitwise(sc, ref_sc, "distributed scalars")
