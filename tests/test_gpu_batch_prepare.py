"""-m gpu: initial configurations prepared on the device (ljmd_batch_prepare, BatchEngine.prepare).  Reproducible mode:
every bit against tests/prepare_model.py (the definition of include/ljmd.h in numpy and Python ints).  fp64 mode:
positions and unscaled velocities against the model bit for bit, forces against the engine's own force call.  Both modes
against the reference's rv_init.dat under bounds derived from its own sums."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import prepare_model as P
import reproducible_model as M
from conftest import GOLDEN, ROOT
from ljmd_amd import BatchEngine, _lib, io_formats, md_types, synthetic
from ljmd_amd._lib import LjmdError
from test_batch_prepare_host import GOLDEN_INPUTS

pytestmark = pytest.mark.gpu

FP64, REPRO = _lib.PRECISION_FP64, _lib.PRECISION_FP64_REPRODUCIBLE
DT = 0.005
# (k, seed): every kernel class (n <= 128, 512, 1024, 2048, 4096) and both class boundaries at 2048 (k = 8 is n = 2048,
# k = 9 the first n above it); k = 3 three times, in different slots and with different seeds
REPLICAS = [(3, 11), (2, 1), (3, -12345), (4, 77), (6, 5), (7, 2024), (8, 3), (9, 99), (3, 1618000)]
WARM = 3


def _params(k):
    n = 4 * k ** 3
    L = synthetic.box_length(n)               # rho = 0.8
    return md_types.init_params(n, L, DT, 0.49 * L)


def _target(p):
    return -4.6 * p.n


def _state(eng):
    """-> per replica {key: [3, n_b]} of the resident state; works for both kinds of engine"""
    st = eng.get_state()
    return [{key: np.stack([np.asarray(st[key][ax][b]) for ax in range(3)]) for key in ("r", "ru", "v", "a")}
            for b in range(eng.n_replicas)]


def _same(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def setup():
    plist = [_params(k) for k, _ in REPLICAS]
    return plist, np.array([s for _, s in REPLICAS], dtype=np.int64), np.array([_target(p) for p in plist])


@pytest.fixture(scope="module")
def model(setup):
    """computed once: steps a-d of every replica in the reproducible mode, and the warm-up of the k <= 4 replicas"""
    plist, seeds, targets = setup
    out = []
    for p, s, t in zip(plist, seeds, targets):
        m = P.prepare(p.n, p.box_length, p.rc, int(s), float(t))
        if p.n <= 256:
            m["warm"] = M.run(m["r"], m["v"], p.box_length, p.dt, p.rc, WARM)
        out.append(m)
    return out


# ---- 1. reproducible mode: every bit is the model's ----------------------------------------------------------------
def test_reproducible_mode_equals_the_model(setup, model):
    plist, seeds, targets = setup
    with BatchEngine.per_replica(plist, precision_mode=REPRO) as eng:
        epot0, ekin0 = eng.prepare(seeds, targets)
        for b, (m, st) in enumerate(zip(model, _state(eng))):
            assert _same(st["r"], m["r"]) and _same(st["ru"], m["r"]), b
            assert _same(st["v"], m["v"]), b
            assert _same(st["a"], m["a"]), b
            assert _same(epot0[b], m["epot0"]) and _same(ekin0[b], m["ekin0"]), (b, epot0[b], m["epot0"])
            assert targets[b] - epot0[b] > 0
        epot_w, ekin_w = eng.prepare(seeds, targets, warmup_steps=WARM)
        assert _same(epot_w, epot0) and _same(ekin_w, ekin0)
        checked = 0
        for b, (m, st) in enumerate(zip(model, _state(eng))):
            assert _same(st["ru"], st["r"]), b
            if "warm" in m:
                w = m["warm"]
                assert _same(st["r"], w["r"]) and _same(st["v"], w["v"]) and _same(st["a"], w["a"]), b
                assert not _same(st["r"], m["r"])
                checked += 1
        assert checked == 5


# ---- 2. fp64 mode ---------------------------------------------------------------------------------------------------
def test_fp64_mode_positions_velocities_and_forces(setup, model):
    plist, seeds, targets = setup
    with BatchEngine.per_replica(plist) as eng:
        epot0, ekin0 = eng.prepare(seeds, targets)
        got = _state(eng)
    for b, (m, st) in enumerate(zip(model, got)):
        assert _same(st["r"], m["r"]) and _same(st["ru"], m["r"]), b
        assert _same(st["v"], m["v0"] * math.sqrt((targets[b] - epot0[b]) / ekin0[b])), b
        assert abs(epot0[b] - m["epot0"]) <= 1e-13 * abs(m["epot0"]) and abs(ekin0[b] - m["ekin0"]) <= 1e-13 * m["ekin0"]
    with BatchEngine.per_replica(plist) as other:
        other.set_state(*[[st["r"][ax] for st in got] for ax in range(3)], *[[st["v"][ax] for st in got] for ax in range(3)])
        epot, _, _ = other.compute_forces()
        want = _state(other)
    assert _same(epot, epot0)
    for b, (st, w) in enumerate(zip(got, want)):
        assert _same(st["a"], w["a"]), b


# ---- 3. against the reference's rv_init.dat -------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [FP64, REPRO])
@pytest.mark.parametrize("name", sorted(GOLDEN_INPUTS))
def test_against_the_reference_rv_init(name, mode):
    n, L, rc, target = GOLDEN_INPUTS[name]
    r_ref, v_ref = io_formats.read_rv_init(GOLDEN / name / "rv_init.dat", n)
    epot_ref = float(np.fromfile(GOLDEN / name / "epot.bin", dtype=np.float64)[0])
    with BatchEngine(md_types.init_params(n, L, 0.002, rc), 1, precision_mode=mode) as eng:
        epot0, _ = eng.prepare(12345, target)
        st = _state(eng)[0]
    assert _same(st["r"], r_ref)
    d_epot = abs(epot0[0] - epot_ref)
    dv = np.abs(st["v"] - v_ref).max()
    vmax = np.abs(v_ref).max()
    bound = (0.5 * d_epot / (target - epot_ref) + n * 2.0 ** -53) * vmax
    print(f"{name} mode {mode}: |epot0 - ref| / |ref| = {d_epot / abs(epot_ref):.3e}, max |dv| = {dv:.3e}, bound {bound:.3e}")
    assert d_epot <= 1e-13 * abs(epot_ref)
    assert dv <= bound


# ---- 4. independence ------------------------------------------------------------------------------------------------
SEED = 42
CHILD = r"""
import sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import numpy as np
import test_gpu_batch_prepare as T
np.save(sys.argv[1], np.stack([T._mixed(int(mode)) for mode in sys.argv[2:]]))
"""


def _trajectory(eng, b, seeds, targets):
    """replica b's prepared state and 20 further steps, as one array of bits"""
    eng.prepare(seeds, targets)
    first = _state(eng)[b]
    sc = eng.steps(20, 5)
    last = _state(eng)[b]
    return np.concatenate([first[k].ravel() for k in ("r", "ru", "v", "a")] + [last[k].ravel() for k in ("r", "ru", "v", "a")] +
                          [s[:, b] for s in sc])


def _mixed(mode):
    """the k = 3 replica in slot 2 of a per-replica handle, between a smaller and two larger systems of other classes"""
    plist = [_params(2), _params(7), _params(3), _params(5)]
    with BatchEngine.per_replica(plist, precision_mode=mode) as eng:
        return _trajectory(eng, 2, [3, 4, SEED, 5], [_target(p) for p in plist])


@pytest.mark.parametrize("mode", [FP64, REPRO])
def test_a_replica_does_not_depend_on_the_others(mode):
    p = _params(3)
    with BatchEngine(p, 1, precision_mode=mode) as eng:
        alone = _trajectory(eng, 0, SEED, _target(p))
    with BatchEngine(p, 3, precision_mode=mode) as eng:
        assert _same(_trajectory(eng, 1, [-SEED, SEED, 9], _target(p)), alone)
        eng.prepare([-SEED, SEED, 9], _target(p))
        st = _state(eng)
        assert _same(st[0]["v"], st[1]["v"])                   # seeds s and -s: one stream
        assert not _same(st[2]["v"], st[1]["v"]) and _same(st[2]["r"], st[1]["r"])
    seeds = np.arange(100, 170)
    seeds[69] = SEED
    with BatchEngine(p, 70, precision_mode=mode) as eng:
        assert _same(_trajectory(eng, 69, seeds, _target(p)), alone)
    assert _same(_mixed(mode), alone)


def test_group_streams_off_in_a_fresh_process(tmp_path):
    out = tmp_path / "mixed.npy"
    subprocess.run([sys.executable, "-c", CHILD % {"root": str(ROOT), "tests": str(ROOT / "tests")}, str(out), str(FP64),
                    str(REPRO)], check=True, timeout=240, env=dict(os.environ, LJMD_BATCH_GROUP_STREAMS="0"))
    got = np.load(out)
    for i, mode in enumerate((FP64, REPRO)):
        assert _same(got[i], _mixed(mode)), mode


# ---- 5. warm-up -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [FP64, REPRO])
@pytest.mark.parametrize("k", [3, 7])
def test_warm_up_is_the_step_path(k, mode):
    p = _params(k)
    seeds, target = [8, 9], _target(p)
    with BatchEngine(p, 2, precision_mode=mode) as eng:
        eng.prepare(seeds, target, warmup_steps=7)
        st = _state(eng)
        assert all(_same(s["ru"], s["r"]) for s in st)
        sc_a = eng.steps(5)
        a = _state(eng)
    with BatchEngine(p, 2, precision_mode=mode) as eng:
        eng.prepare(seeds, target)
        assert not _same(_state(eng)[0]["r"], st[0]["r"])
        sc_b = eng.steps(12)
        b = _state(eng)
    for x, y in zip(a, b):
        assert _same(x["r"], y["r"]) and _same(x["v"], y["v"]) and _same(x["a"], y["a"])
    for x, y in zip(sc_a, sc_b):
        assert _same(x, y[7:])


def test_warm_up_takes_no_snapshot():
    p = _params(3)
    with BatchEngine(p, 2) as eng:
        eng.rdf_configure(32, every=1)
        eng.tcf_configure(4, 1, every=1)
        eng.prepare([1, 2], _target(p), warmup_steps=4)
        assert eng.rdf_read()[1] == 0 and eng.tcf_read()[3] == 0
        assert not eng.rdf_read()[0].any()
        eng.steps(2, observables=False)
        assert eng.rdf_read()[1] == 2 and eng.tcf_read()[3] == 2
        assert eng.tcf_read()[2].tolist() == [1, 1, 0, 0, 0]      # numbered from 0 after prepare: lag 1 once


# ---- 6. errors ------------------------------------------------------------------------------------------------------
def test_a_target_below_the_lattice_energy():
    plist = [_params(3), _params(1), _params(2)]
    targets = [_target(p) for p in plist]                          # k = 1: n = 4, target -18.4
    with BatchEngine.per_replica(plist) as eng:
        with pytest.raises(LjmdError) as ei:
            eng.prepare(5, targets)
        assert ei.value.code == _lib.LJMD_ERR_INVALID_ARG and "replica 1:" in ei.value.message
        with pytest.raises(LjmdError) as e2:
            eng.steps(1)
        assert e2.value.code == _lib.LJMD_ERR_STATE and "no state" in e2.value.message
        r = [P.lattice(p.n, p.box_length) for p in plist]
        v = [P.velocities(p.n, 3) for p in plist]
        eng.set_state(*[[x[ax] for x in r] for ax in range(3)], *[[x[ax] for x in v] for ax in range(3)])
        epot, _, _ = eng.compute_forces()
        print("k = 1: target - epot0 =", targets[1] - epot[1])
        assert targets[1] - epot[1] < 0 < targets[0] - epot[0]
        assert np.isfinite(eng.steps(1)[0]).all()


def test_argument_errors_leave_the_handle_alone():
    L = synthetic.box_length(500)
    with BatchEngine.per_replica([md_types.init_params(500, L, DT, 0.49 * L), md_types.init_params(100, L, DT, 0.49 * L)]) as eng:
        with pytest.raises(LjmdError) as ei:
            eng.prepare(1, -4.6 * 500)
        assert ei.value.code == _lib.LJMD_ERR_INVALID_ARG and "replica 1:" in ei.value.message and "100" in ei.value.message
    p = _params(3)
    with BatchEngine(p, 2) as eng:
        eng.prepare([1, 2], _target(p))
        before = _state(eng)
        for seeds, warm in (([1, -2 ** 31], 0), ([1, 2], -1)):
            with pytest.raises(LjmdError) as ei:
                eng.prepare(seeds, _target(p), warmup_steps=warm)
            assert ei.value.code == _lib.LJMD_ERR_INVALID_ARG
        lib = _lib.load()
        t = np.full(2, _target(p))
        s = np.ones(2, dtype=np.int32)
        assert lib.ljmd_batch_prepare(eng._h, None, t.ctypes.data_as(_lib.c_double_p), 0, None, None) == _lib.LJMD_ERR_INVALID_ARG
        assert lib.ljmd_batch_prepare(eng._h, s.ctypes.data_as(_lib.c_int32_p), None, 0, None, None) == _lib.LJMD_ERR_INVALID_ARG
        assert lib.ljmd_batch_prepare(eng._h, s.ctypes.data_as(_lib.c_int32_p), t.ctypes.data_as(_lib.c_double_p), 0, None,
                                      None) == _lib.LJMD_OK        # epot0 and ekin0 may be NULL
        eng.prepare([1, 2], _target(p))
        for x, y in zip(before, _state(eng)):
            assert all(_same(x[key], y[key]) for key in ("r", "ru", "v", "a"))
        assert np.isfinite(eng.steps(1)[0]).all()
