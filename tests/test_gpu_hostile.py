"""-m gpu: the pair kernels on inhomogeneous and raw-coordinate inputs (tests/hostile_configs.py, whose properties
tests/test_hostile_configs.py proves on the CPU): a droplet in vapour wrapped through three faces, a slab in vacuum across
a face, two monolayers with two z values, and the same systems in raw periodic images spanning just under 2.4 L.  Tile
extents differ by an order of magnitude, some boxes have zero width, whole regions of the tile-pair mask are empty.

Every particle is compared.  Bounds against the pinned oracle are the project's own at these sizes: scalars 1e-12
relative, accelerations 1e-12 max|a_oracle|, step series 1e-10 relative (test_gpu_parity.py); integer results are equal.
One wrongly skipped pair inside the cutoff exceeds every one of them (test_hostile_configs.py)."""
import functools

import numpy as np
import pytest

import heatflux_model
import hostile_configs as hc
import reproducible_model as M
import stress_model
from ljmd_amd import BatchEngine, Engine, _lib, init_params, synthetic

pytestmark = pytest.mark.gpu

REL_SCALAR = 1e-12
REL_ACCEL = 1e-12
REL_TRAJ = 1e-10
MODE_REPRO = _lib.PRECISION_FP64_REPRODUCIBLE

# raw coordinate spans (in L, any axis) at which set_state switches: from 1.4 L on the Newton-3 kernels' frame per row group
# is taken from wrapped coordinates (else it would reach L / 2 beyond the raw span), from 2.4 L on the generic kernel takes
# the evaluations before the first wrap
N3_SPAN, GATHER_SPAN = 1.4, 2.4


def _with_rc(cfg, rc_over_L):
    p, r, v = cfg
    return init_params(p.n, p.box_length, p.dt, rc_over_L * p.box_length), r, v


@functools.lru_cache(maxsize=None)
def config(name):
    """the shared inputs, built once and never written to"""
    make = {
        "droplet": lambda: hc.droplet(hc.DROPLET_S),
        "slab": lambda: hc.slab(hc.SLAB_S),
        "sheets": lambda: hc.sheets(hc.SHEETS_S),
        "raw_droplet": lambda: hc.raw_images(config("droplet")),
        "raw_slab": lambda: hc.raw_images(config("slab")),
        "droplet_rc15": lambda: _with_rc(config("droplet"), 0.15),
        "slab_rc15": lambda: _with_rc(config("slab"), 0.15),
        "sheets_rc15": lambda: _with_rc(config("sheets"), 0.15),
        "raw_droplet_rc15": lambda: _with_rc(config("raw_droplet"), 0.15),
        "raw_slab_rc15": lambda: _with_rc(config("raw_slab"), 0.15),
        "droplet_M": lambda: hc.droplet(hc.DROPLET_M),
        "raw_slab_M": lambda: hc.raw_images(hc.slab(hc.SLAB_M)),
        "below_n3_span": lambda: _at_span(config("droplet"), N3_SPAN, above=()),
        "at_n3_span": lambda: _at_span(config("droplet"), N3_SPAN, above=(2,)),
        "framed_beyond_span": lambda: _framed_beyond_span(config("droplet")),
    }[name]
    p, r, v = make()
    r.setflags(write=False)
    v.setflags(write=False)
    return p, r, v


def _at_span(cfg, span_over_L, above):
    """The configuration in raw images spanning 1 ulp less than span_over_L L on every axis -- (hi - lo) < span_over_L * L
    in the doubles set_state computes -- or, on the axes in `above`, the first span for which that is false.  Whole-L moves
    inside (-0.19 L, 1.1 L) for everybody; then per axis two particles A (0.7 to 0.81 L, moved down by L) and B (0.1 to 0.21 L,
    moved up by L) chosen so that B - A + 2 L is as close to the span as the configuration allows, and B nudged (by less
    than 1e-3 sigma) onto the threshold."""
    p, r, v = cfg
    L = p.box_length
    _, x, _ = hc.raw_images(cfg, seed=505, lo=-0.19, hi=1.10)
    x = x.copy()
    target = span_over_L * L
    for ax in range(3):
        ia = np.flatnonzero((r[ax] > 0.70 * L) & (r[ax] < 0.81 * L))
        ib = np.flatnonzero((r[ax] > 0.10 * L) & (r[ax] < 0.21 * L))
        miss = np.abs((r[ax][ib][None, :] + L) - (r[ax][ia][:, None] - L) - target)
        i, j = np.unravel_index(np.argmin(miss), miss.shape)
        assert miss[i, j] < 1e-3
        lo = r[ax][ia[i]] - L
        hi = lo + target
        while hi - lo < target:
            hi = np.nextafter(hi, np.inf)
        if ax not in above:
            while not hi - lo < target:
                hi = np.nextafter(hi, -np.inf)
        x[ax, ia[i]], x[ax, ib[j]] = lo, hi
        assert x[ax].min() == lo and x[ax].max() == hi and (hi - lo < target) == (ax not in above)
    return p, np.ascontiguousarray(x), v.copy()


def _framed_beyond_span(cfg):
    """The droplet in the caller's order and raw images that put two tiles of the Newton-3 kernels' framed copy L / 2
    beyond the raw span (2.3 L in z, below the 2.4 L the gather kernels need).  With two-tile row groups and no sort, slots
    0..127 and 128..255 are row groups.  Group 0: its first particle P (z near 0.35 L) moved down by L, and as its second
    tile 64 droplet particles with z in (0.90, 0.98) L moved down by L: they lie 0.55 to 0.63 L above P, so the frame of
    the group puts them another L down, at (-1.10, -1.02) L.  Group 1 mirrors it: Q (z near 0.65 L) moved up by L, second
    tile from z in (0.02, 0.10) L moved up by L, framed at (2.02, 2.10) L.  The two tiles are neighbours through the z face
    (0.04 to 0.2 L apart) while their framed boxes differ by 3.04 to 3.2 L."""
    p, r, v = cfg
    L, n = p.box_length, p.n
    z = r[2]
    d = r[:2] - L * np.rint(r[:2] / L)
    rho2 = np.sum(d * d, axis=0)                           # squared distance from the z axis through the corner

    def pick(lo, hi, count, taken):
        idx = np.flatnonzero((z > lo * L) & (z < hi * L))
        idx = idx[~np.isin(idx, taken)]
        assert idx.size >= count
        return idx[np.argsort(rho2[idx], kind="stable")[:count]]

    a1 = pick(0.90, 0.98, 64, [])
    b1 = pick(0.02, 0.10, 64, [])
    pp = pick(0.33, 0.37, 1, [])
    qq = pick(0.63, 0.67, 1, [])
    used = np.concatenate([a1, b1, pp, qq])
    rest = np.setdiff1d(np.arange(n), used)
    order = np.concatenate([pp, rest[:63], a1, qq, rest[63:126], b1, rest[126:]])
    assert order.size == n and np.unique(order).size == n
    x = r.copy()
    x[2, pp] -= L
    x[2, a1] -= L
    x[2, qq] += L
    x[2, b1] += L
    return p, np.ascontiguousarray(x[:, order]), np.ascontiguousarray(v[:, order])


def _oracle_params(oracle, p):
    return oracle.derive_params(p.n, p.box_length, p.dt, p.rc)


_force_cache, _traj_cache = {}, {}


def _oracle_threads():
    """the oracle's OpenMP form on the CPUs this process may use (as test_gpu_parity.py: oracle_rows_n262144)"""
    import ctypes
    import os
    cores = len(os.sched_getaffinity(0))
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            cores = min(cores, max(1, int(quota) // int(period)))
    except (OSError, ValueError):
        pass
    try:
        ctypes.CDLL("libgomp.so.1").omp_set_num_threads(min(cores, 16))
    except OSError:
        pass


def oracle_at(oracle, p, r):
    """-> (epot, d_epot, dd_epot, a[3, n]): the oracle over all ordered pairs (rows independent, the reference's per-pair
    arithmetic), every unordered pair seen twice"""
    _oracle_threads()
    po = _oracle_params(oracle, p)
    ax, ay, az, se, sd, sdd = oracle.rows_raw(po, 0, p.n, r[0].copy(), r[1].copy(), r[2].copy())
    te, td, tdd = oracle.tail_corrections(po)
    return 4.0 * (0.5 * se) + te, 24.0 * (0.5 * sd) + td, 24.0 * (0.5 * sdd) + tdd, 24.0 * np.stack([ax, ay, az])


def oracle_force(oracle, name):
    """oracle_at of a shared configuration, computed once"""
    if name not in _force_cache:
        p, r, v = config(name)
        _force_cache[name] = oracle_at(oracle, p, r)
    return _force_cache[name]


def oracle_traj(oracle, name, nsteps):
    """-> (scalars[nsteps, 4], final state dict) of oracle.run_steps from a shared configuration, computed once"""
    if (name, nsteps) not in _traj_cache:
        p, r, v = config(name)
        a = oracle_force(oracle, name)[3]
        st = {"rx": r[0].copy(), "ry": r[1].copy(), "rz": r[2].copy(), "ux": r[0].copy(), "uy": r[1].copy(), "uz": r[2].copy(),
              "vx": v[0].copy(), "vy": v[1].copy(), "vz": v[2].copy(), "ax": a[0].copy(), "ay": a[1].copy(), "az": a[2].copy()}
        _traj_cache[name, nsteps] = (oracle.run_steps(_oracle_params(oracle, p), nsteps, st), st)
    return _traj_cache[name, nsteps]


def rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


def check_force(tag, sc, a, ref, scalar=REL_SCALAR, accel=REL_ACCEL, floor=0.0):
    dev = [rel(x, y) for x, y in zip(sc, ref[:3])] + [np.abs(a - ref[3]).max() / np.abs(ref[3]).max()]
    print(f"{tag}: epot, d_epot, dd_epot rel {dev[0]:.2e} {dev[1]:.2e} {dev[2]:.2e}, max|da| / max|a| {dev[3]:.2e}")
    assert max(dev[:3]) <= scalar, (tag, dev)
    assert np.abs(a - ref[3]).max() <= accel * np.abs(ref[3]).max() + floor, (tag, dev)


def set_state(eng, r, v):
    eng.set_state(r[0], r[1], r[2], v[0], v[1], v[2])


def force_call(p, r, v, **kw):
    with Engine(p, **kw) as eng:
        set_state(eng, r, v)
        name = eng.pair_kernel_name()
        sc = eng.compute_forces()
        a = np.stack(eng.get_state(("a",))["a"])
    return name, sc, a


def expected_kernel(name, n3=True):
    """which pair kernel serves the first evaluation of a shared configuration"""
    p, r, v = config(name)
    span = ((r.max(axis=1) - r.min(axis=1)) / p.box_length).max()
    if span >= GATHER_SPAN:
        return "pair_rows_generic_kernel"
    return "pair_n3_kernel" if n3 else "pair_tiles_kernel"


# ---- a. fp64 force parity at t = 0, S ---------------------------------------------------------------------------------
PATHS = {"default": {}, "rt2": {"LJMD_N3_ROW_TILES": "2"}, "rt4": {"LJMD_N3_ROW_TILES": "4"}, "gather": {"LJMD_N3": "0"}}


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("name", ["droplet", "slab", "sheets", "raw_droplet"])
def test_force_parity_s(oracle, name, path, monkeypatch):
    """One force call per configuration and kernel path: the default Newton-3 kernel (one tile per row group at this size),
    two- and four-tile row groups (tile_class_kernel, cluster passes, per-tile images), and the gather kernel.  Raw input
    spanning 2.38 L: the gather kernel walks tiles of the raw coordinates (|d| < 2.4 L), the Newton-3 kernels tiles framed
    from the wrapped ones."""
    for k, val in PATHS[path].items():
        monkeypatch.setenv(k, val)
    p, r, v = config(name)
    kernel, sc, a = force_call(p, r, v)
    check_force(f"{name} {path} ({kernel})", sc, a, oracle_force(oracle, name))
    assert kernel == expected_kernel(name, n3=path != "gather")


@pytest.mark.parametrize("name", ["droplet_rc15", "raw_droplet_rc15"])
def test_force_parity_s_short_cutoff(oracle, name):
    """rc = 0.15 L: 42 % of the tile pairs lie beyond the cutoff, so a wrong box gap drops pairs here first."""
    p, r, v = config(name)
    kernel, sc, a = force_call(p, r, v)
    check_force(f"{name} ({kernel})", sc, a, oracle_force(oracle, name))
    assert kernel == expected_kernel(name)


@pytest.mark.parametrize("name,path,rc_over_L", [
    ("below_n3_span", "default", 0.49), ("below_n3_span", "default", 0.15), ("below_n3_span", "rt2", 0.49),
    ("below_n3_span", "rt2", 0.15), ("below_n3_span", "rt4", 0.49), ("below_n3_span", "rt4", 0.15),
    ("at_n3_span", "default", 0.49), ("at_n3_span", "default", 0.15)])
def test_raw_span_either_side_of_the_newton3_limit(oracle, name, path, rc_over_L, monkeypatch):
    """The droplet in raw images whose span is one ulp below 1.4 L on every axis -- the widest input whose raw coordinates
    the Newton-3 kernels frame: row groups up to 0.7 L wide, framed positions up to L / 2 outside the span, box differences
    up to 2.4 L -- and with the z span exactly at the limit, from where the wrapped coordinates are framed."""
    for k, val in PATHS[path].items():
        monkeypatch.setenv(k, val)
    p, r, v = _with_rc(config(name), rc_over_L)
    span = r.max(axis=1) - r.min(axis=1)
    assert np.all(span > 1.399 * p.box_length)
    got, sc, a = force_call(p, r, v)
    check_force(f"{name} {path} rc = {rc_over_L} L ({got})", sc, a, oracle_at(oracle, p, r))
    assert got == "pair_n3_kernel"


@pytest.mark.parametrize("groups", ["2", "4"])
def test_row_group_framed_beyond_the_raw_span(oracle, groups, monkeypatch):
    """Row groups in the caller's order (no sort), raw z spanning 2.33 L, arranged so that a frame of the raw coordinates
    carries two neighbouring tiles to box differences of 3.04 to 3.2 L, where axis_gap (|d| < 2.5 L, m = -2..2) reports a gap
    of 1.04 L for a true one of 0.04 L and the tile pair was dropped (epot off by 4e-4).  From a span of 1.4 L on the frame is
    taken from the wrapped coordinates.  (Four-tile groups: the same two tiles, now inside ONE group.)"""
    monkeypatch.setenv("LJMD_SORT", "0")
    monkeypatch.setenv("LJMD_N3_ROW_TILES", groups)
    p, r, v = config("framed_beyond_span")
    span = (r.max(axis=1) - r.min(axis=1)) / p.box_length
    assert span.max() < GATHER_SPAN and 2.25 < span[2] < 2.35
    kernel, sc, a = force_call(p, r, v)
    check_force(f"framed_beyond_span, {groups}-tile groups ({kernel})", sc, a, oracle_force(oracle, "framed_beyond_span"))
    assert kernel == "pair_n3_kernel"


# ---- b. the same at M --------------------------------------------------------------------------------------------------
M_PATHS = {"default": {}, "rt4": {"LJMD_N3_ROW_TILES": "4"},
           "rt4_no_clusters": {"LJMD_N3_ROW_TILES": "4", "LJMD_N3_CLUSTERS": "0"},
           "rt4_no_pertile": {"LJMD_N3_ROW_TILES": "4", "LJMD_N3_PERTILE": "0"}}


@pytest.mark.parametrize("path", list(M_PATHS))
@pytest.mark.parametrize("name", ["droplet_M", "raw_slab_M"])
def test_force_parity_m(oracle, name, path, monkeypatch):
    """16 500 <= n <= 20 000: the plan takes two-tile row groups and the two-launch step by itself (the default's bits are
    those of LJMD_N3_ROW_TILES=2); four-tile groups use the separate tile_class_kernel, cluster passes and per-tile images,
    each also switched off.  The raw slab spans 2.36 L in y and z and 1.28 L, with a gap of 0.7 L, in x."""
    for k, val in M_PATHS[path].items():
        monkeypatch.setenv(k, val)
    p, r, v = config(name)
    kernel, sc, a = force_call(p, r, v)
    check_force(f"{name} {path} ({kernel})", sc, a, oracle_force(oracle, name))
    assert kernel == expected_kernel(name)
    if path == "default" and kernel == "pair_n3_kernel":
        monkeypatch.setenv("LJMD_N3_ROW_TILES", "2")
        kernel2, sc2, a2 = force_call(p, r, v)
        assert kernel2 == kernel and sc2 == sc and np.array_equal(a2, a), "the default plan at M is not the two-tile one"


# ---- c. moving tiles ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("resort", ["1000", "1"])
@pytest.mark.parametrize("name", ["droplet", "slab"])
def test_twelve_steps_then_forces_at_the_engines_positions(oracle, name, resort, monkeypatch):
    """12 steps without any re-sort (tiles deform, particles cross the faces the dense part lies on) and with a re-sort every
    step; the series against oracle.run_steps, then e, d, dd and a against the oracle at the engine's own positions."""
    monkeypatch.setenv("LJMD_RESORT_EVERY", resort)
    p, r, v = config(name)
    with Engine(p) as eng:
        set_state(eng, r, v)
        assert eng.pair_kernel_name() == "pair_n3_kernel"
        eng.compute_forces()
        sc = np.stack(eng.verlet_steps(12), axis=1)
        st = eng.get_state(("r", "a"))
    sc_o, _ = oracle_traj(oracle, name, 12)
    dev = np.max(np.abs(sc - sc_o) / np.abs(sc_o), axis=0)
    print(f"{name} resort every {resort}: 12-step series rel (epot, ekin, d, dd) {dev}")
    assert dev.max() <= REL_TRAJ
    rr, a = np.stack(st["r"]), np.stack(st["a"])
    assert rr.min() >= 0.0 and rr.max() <= p.box_length
    check_force(f"{name} resort every {resort}, after 12 steps", sc[-1, [0, 2, 3]], a, oracle_at(oracle, p, rr))


def test_sheets_resort_every_step_keeps_particle_identity(oracle, monkeypatch):
    """Tile boxes of zero z width through a re-sort per step: get_state returns the caller's order, and ru - r is a whole
    number of box lengths for the same particle."""
    monkeypatch.setenv("LJMD_RESORT_EVERY", "1")
    p, r, v = config("sheets")
    with Engine(p) as eng:
        set_state(eng, r, v)
        st0 = eng.get_state(("r", "ru", "v"))
        assert all(np.array_equal(np.stack(st0[k]), x) for k, x in (("r", r), ("ru", r), ("v", v)))
        eng.compute_forces()
        sc = np.stack(eng.verlet_steps(12), axis=1)
        st = eng.get_state(("r", "ru", "a"))
    rr, ru, a = (np.stack(st[k]) for k in ("r", "ru", "a"))
    k = (ru - rr) / p.box_length
    assert np.abs(k - np.rint(k)).max() < 1e-9
    assert np.abs(ru - r).max() < 0.5                    # 12 steps: nobody moved far, so every column is still its particle
    sc_o, fin = oracle_traj(oracle, "sheets", 12)
    assert np.max(np.abs(sc - sc_o) / np.abs(sc_o)) <= REL_TRAJ
    assert np.abs(ru - np.stack([fin["ux"], fin["uy"], fin["uz"]])).max() <= 1e-10
    check_force("sheets resort every step, after 12 steps", sc[-1, [0, 2, 3]], a, oracle_at(oracle, p, rr))


# ---- d. raw input through a step ---------------------------------------------------------------------------------------
def test_raw_input_through_three_steps(oracle):
    p, r, v = config("raw_droplet")
    with Engine(p) as eng:
        set_state(eng, r, v)
        first = eng.compute_forces()
        sc = np.stack(eng.verlet_steps(3), axis=1)
        assert eng.pair_kernel_name() == "pair_n3_kernel"
        st = eng.get_state(("r", "ru"))
    ref = oracle_force(oracle, "raw_droplet")
    assert max(rel(x, y) for x, y in zip(first, ref[:3])) <= REL_SCALAR
    sc_o, fin = oracle_traj(oracle, "raw_droplet", 3)
    dev = np.max(np.abs(sc - sc_o) / np.abs(sc_o), axis=0)
    print(f"raw_droplet: 3-step series rel (epot, ekin, d, dd) {dev}")
    assert dev.max() <= REL_TRAJ
    rr, ru = np.stack(st["r"]), np.stack(st["ru"])
    assert rr.min() >= 0.0 and rr.max() <= p.box_length
    assert np.abs(ru - np.stack([fin["ux"], fin["uy"], fin["uz"]])).max() <= 1e-10


# ---- e. reproducible mode, bitwise -------------------------------------------------------------------------------------
def bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)


def assert_bitwise(a, b, what):
    ba, bb = bits(a), bits(b)
    assert ba.shape == bb.shape, what
    bad = np.flatnonzero(ba.ravel() != bb.ravel())
    assert bad.size == 0, (what, bad.size, np.ravel(a)[bad[:4]], np.ravel(b)[bad[:4]])


def _repro_run(p, r, v, nsteps):
    with Engine(p, precision_mode=MODE_REPRO) as eng:
        set_state(eng, r, v)
        assert eng.pair_kernel_name() == "pair_fixed_kernel"
        first = eng.compute_forces()
        a0 = np.stack(eng.get_state(("a",))["a"])
        sc = np.stack(eng.verlet_steps(nsteps), axis=1)
        st = eng.get_state()
    return first, a0, sc, {k: np.stack(st[k]) for k in ("r", "ru", "v", "a")}


@functools.lru_cache(maxsize=None)
def _repro_reference(name):
    p, r, v = config(name)
    return _repro_run(p, r, v, 10)


@pytest.mark.parametrize("env", [{}, {"LJMD_RESORT_EVERY": "1"}, {"LJMD_SORT": "0"}, {"LJMD_FORCE_GENERIC": "1"}],
                         ids=["default", "resort1", "nosort", "generic"])
@pytest.mark.parametrize("name", ["droplet", "sheets", "raw_slab"])
def test_reproducible_mode_bitwise_across_knobs(oracle, name, env, monkeypatch):
    """Integer sums: with the tile-pair mask (default), a new tile set every step, the caller's order (every tile meets every
    tile that the boxes allow) and no mask at all (LJMD_FORCE_GENERIC walks every tile pair), t = 0 scalars, a(0), the 10-step
    series and r, ru, v, a must be the same words -- one wrongly skipped pair inside the cutoff changes them.  The default's
    t = 0 result is also held against the oracle."""
    ref = _repro_reference(name)
    if not env:
        check_force(f"{name} reproducible t = 0", ref[0], ref[1], oracle_force(oracle, name))
        return
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    p, r, v = config(name)
    first, a0, sc, st = _repro_run(p, r, v, 10)
    what = f"{name} {env}"
    assert_bitwise(first, ref[0], what + " t = 0")
    assert_bitwise(a0, ref[1], what + " a(0)")
    assert_bitwise(sc, ref[2], what + " series")
    for k in st:
        assert_bitwise(st[k], ref[3][k], what + " " + k)


# ---- f. mixed precision ------------------------------------------------------------------------------------------------
def test_mixed_precision_droplet_m(oracle):
    """The vapour tiles are wide, so their fp32 offsets from the tile centre are coarse; bounds as written in include/ljmd.h
    and used in test_liquid_state_forces_vs_oracle_n65536 (24 rc^-7 for a pair on the cutoff edge)."""
    p, r, v = config("droplet_M")
    ref = oracle_force(oracle, "droplet_M")
    kernel, sc, a = force_call(p, r, v, precision_mode=_lib.PRECISION_FP32_FORCE)
    assert kernel == "pair_n3_f32_kernel"
    edge = 24.0 * abs(p.rc ** -7 - 2.0 * p.rc ** -13)
    check_force("droplet_M mixed", sc, a, ref, scalar=5e-9, accel=1e-9, floor=2.0 * edge)


# ---- g. resident g(r) and stress walks ---------------------------------------------------------------------------------
@pytest.mark.parametrize("rmax_over_L", [0.5, 0.15])
@pytest.mark.parametrize("name", ["droplet", "slab", "sheets"])
def test_rdf_walk_counts_equal_the_oracle(oracle, name, rmax_over_L):
    p, r, v = config(name)
    L, nbins = p.box_length, 200
    with Engine(p) as eng:
        set_state(eng, r, v)
        eng.compute_forces()
        eng.rdf_configure(nbins, rmax_over_L * L)
        eng.rdf_accumulate()
        hist, count = eng.rdf_read()
        prof = eng.rdf_profile()
        x, y, z = eng.get_state(("r",))["r"]
    assert count == 1 and np.array_equal(np.stack([x, y, z]), r)
    want = np.zeros(nbins, dtype=np.uint64)
    oracle.rdf_histogram_np(np.ascontiguousarray(x), np.ascontiguousarray(y), np.ascontiguousarray(z), L, nbins, rmax_over_L * L, want)
    print(f"g(r) {name} rmax = {rmax_over_L} L: tile pairs visited {prof['tile_pairs_visited']} of {prof['tile_pairs_total']}")
    assert np.array_equal(hist, want), np.flatnonzero(hist != want)[:8]
    assert hist.sum() > 0
    assert 0 < prof["tile_pairs_visited"] < prof["tile_pairs_total"], prof


@pytest.mark.parametrize("name", ["droplet", "slab", "sheets", "droplet_rc15", "slab_rc15", "sheets_rc15", "raw_droplet_rc15",
                                  "raw_slab_rc15"])
def test_stress_walk_words_equal_the_model(name):
    """the raw names: spans of 2.38 L (droplet) and 1.27, 2.35, 2.35 L (slab), below the 2.4 L at which skipping switches
    off, so box differences approach the 2.5 L that rdf_axis_gap covers"""
    p, r, v = config(name)
    with Engine(p) as eng:
        set_state(eng, r, v)
        eng.compute_forces()
        eng.stress_configure(1)
        eng.stress_accumulate()
        words = eng.stress_read_exact()
        prof = eng.stress_profile()
    want, flag = stress_model.words(r, v, p.box_length, p.rc)
    print(f"stress {name}: tile pairs visited {prof['tile_pairs_visited']} of {prof['tile_pairs_total']}")
    assert not flag and words.shape == (1, 12)
    assert list(words[0]) == want, [c for c in range(12) if words[0][c] != want[c]]
    assert 0 < prof["tile_pairs_visited"] < prof["tile_pairs_total"], prof


@pytest.mark.parametrize("name", ["droplet_rc15", "slab_rc15", "sheets_rc15", "raw_droplet_rc15", "raw_slab_rc15"])
def test_heatflux_walk_words_equal_the_model(name):
    """heatflux_pairs_kernel has its own copy of the walk and reads the velocities from the column side as well.  sheets:
    every tile box has zero width in z and every velocity pair is still distinct.  The pressure tensor accumulated on the
    same engine must have visited the same tile pairs: the same bound on the same boxes"""
    p, r, v = config(name)
    with Engine(p) as eng:
        set_state(eng, r, v)
        eng.compute_forces()
        eng.heatflux_configure(1)
        eng.heatflux_accumulate()
        words = eng.heatflux_read_exact()
        prof = eng.heatflux_profile()
        eng.stress_configure(1)
        eng.stress_accumulate()
        sprof = eng.stress_profile()
        st = eng.get_state(("r", "v"))
    assert np.array_equal(np.stack(st["r"]), r) and np.array_equal(np.stack(st["v"]), v)
    want, flag = heatflux_model.words(r, v, p.box_length, p.rc)
    print(f"heatflux {name}: tile pairs visited {prof['tile_pairs_visited']} of {prof['tile_pairs_total']}")
    assert not flag and words.shape == (1, 9)
    assert list(words[0]) == want, [heatflux_model.ROWS[c] for c in range(9) if words[0][c] != want[c]]
    assert all(w != 0 for w in want)
    assert 0 < prof["tile_pairs_visited"] < prof["tile_pairs_total"], prof
    assert (sprof["tile_pairs_visited"], sprof["tile_pairs_total"]) == (prof["tile_pairs_visited"], prof["tile_pairs_total"])


# ---- h. sharded on one card --------------------------------------------------------------------------------------------
def test_slab_sharded_four_ranks_one_card(oracle):
    """index-range shards of the shuffled slab: every rank's own shard is slab-shaped, and its k-d sort splits y and z only"""
    p, r, v = config("slab")
    assert p.n % 4 == 0
    kernel, sc, a = force_call(p, r, v, devices=[0] * 4)
    check_force(f"slab, 4 ranks ({kernel})", sc, a, oracle_force(oracle, "slab"))
    assert kernel == "pair_n3_kernel"


# ---- i. batch engine ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _raw_replicas(n):
    """-> params, x[3, 3, n], v[3, 3, n]: raw images (spans 2.2 to 2.3 L) of three make_config systems"""
    cfg = [hc.raw_images(synthetic.make_config(n, seed=s), seed=600 + s) for s in (51, 52, 53)]
    return cfg[0][0], np.stack([c[1] for c in cfg]), np.stack([c[2] for c in cfg])


def _batch_set(eng, x, v):
    eng.set_state(x[:, 0], x[:, 1], x[:, 2], v[:, 0], v[:, 1], v[:, 2])


@pytest.mark.parametrize("n", [500, 1372])
def test_batch_raw_input_fp64(oracle, n):
    """one and two particles per thread; forces and scalars at the bounds of test_gpu_batch.py, 5 steps of series"""
    p, x, v = _raw_replicas(n)
    po = _oracle_params(oracle, p)
    with BatchEngine(p, 3) as eng:
        _batch_set(eng, x, v)
        e, d, dd = eng.compute_forces()
        a = np.stack(eng.get_state(("a",))["a"], axis=1)
        sc = np.stack(eng.steps(5, sample_every=1), axis=2)              # [5, B, 4]
    for b in range(3):
        ref = oracle_at(oracle, p, x[b])
        check_force(f"batch n = {n} replica {b}", (e[b], d[b], dd[b]), a[b], ref, scalar=1e-13)
        st = {"rx": x[b, 0].copy(), "ry": x[b, 1].copy(), "rz": x[b, 2].copy(), "ux": x[b, 0].copy(), "uy": x[b, 1].copy(),
              "uz": x[b, 2].copy(), "vx": v[b, 0].copy(), "vy": v[b, 1].copy(), "vz": v[b, 2].copy(),
              "ax": ref[3][0].copy(), "ay": ref[3][1].copy(), "az": ref[3][2].copy()}
        sc_o = oracle.run_steps(po, 5, st)
        assert np.max(np.abs(sc[:, b] - sc_o) / np.abs(sc_o)) <= REL_TRAJ, b


@pytest.mark.parametrize("n", [500, 1372])
def test_batch_raw_input_reproducible_equals_the_model(n):
    p, x, v = _raw_replicas(n)
    nsteps = 5
    with BatchEngine(p, 3, precision_mode=MODE_REPRO) as eng:
        _batch_set(eng, x, v)
        first = eng.compute_forces()
        sc = np.stack(eng.steps(nsteps, sample_every=1), axis=2)
        st = eng.get_state()
    for b in range(3):
        m = M.run(x[b], v[b], p.box_length, p.dt, p.rc, nsteps)
        assert_bitwise([f[b] for f in first], m["first"], f"replica {b} t = 0")
        assert_bitwise(sc[:, b], m["scalars"], f"replica {b} series")
        for key in ("r", "ru", "v", "a"):
            assert_bitwise(np.stack(st[key], axis=1)[b], m[key], f"replica {b} {key}")
