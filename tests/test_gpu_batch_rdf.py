"""-m gpu: g(r) histograms accumulated on the device by the batch engine (ljmd_batch_rdf_*, BatchEngine.rdf_*).  The
counts are integers: every comparison is equality with oracle.rdf_histogram_np (the reference's numpy arithmetic) on the
positions get_state returns, per replica with its own n, L and rmax."""
import numpy as np
import pytest

from ljmd_amd import BatchEngine, _lib, analysis, md_types, synthetic
from ljmd_amd._lib import LjmdError

pytestmark = pytest.mark.gpu


def _oracle_hist(oracle, x, y, z, L, nbins, rmax):
    h = np.zeros(nbins, dtype=np.uint64)
    oracle.rdf_histogram_np(np.asarray(x), np.asarray(y), np.asarray(z), L, nbins, rmax, h)
    return h


def _replicas(n, seeds):
    cfg = [synthetic.make_config(n, seed=s) for s in seeds]
    return cfg[0][0], np.stack([c[1] for c in cfg]), np.stack([c[2] for c in cfg])       # p, r[B, 3, n], v[B, 3, n]


def _set(eng, r, v):
    eng.set_state(r[:, 0], r[:, 1], r[:, 2], v[:, 0], v[:, 1], v[:, 2])


# ---- 1. one-shot accumulate, homogeneous handles ---------------------------------------------------------------------
# every kernel class (<= 128, 512, 1024, 2048, 4096), partial waves, the two- and four-particles-per-thread mappings,
# the smallest system; nbins = 8192 at n = 4096 is the largest LDS footprint; rmax_over_L None = the default 0.5 L
@pytest.mark.parametrize("n, B, nbins, rmax_over_L", [
    (2, 3, 200, None), (65, 3, 200, None), (108, 3, 200, None), (500, 3, 200, None), (1025, 3, 200, None),
    (2049, 2, 200, None), (4096, 2, 200, None), (4096, 2, 8192, None), (500, 3, 200, 0.3),
])
def test_one_shot_counts_equal_the_oracle(oracle, n, B, nbins, rmax_over_L):
    p, r, v = _replicas(n, range(100, 100 + B))
    L = p.box_length
    rmax = None if rmax_over_L is None else rmax_over_L * L
    with BatchEngine(p, B) as eng:
        _set(eng, r, v)
        eng.rdf_configure(nbins, rmax=rmax)
        eng.rdf_accumulate()
        hist, count = eng.rdf_read()
        x, y, z = eng.get_state(("r",))["r"]
    assert count == 1 and hist.shape == (B, nbins) and hist.dtype == np.uint64
    for b in range(B):
        want = _oracle_hist(oracle, x[b], y[b], z[b], L, nbins, 0.5 * L if rmax is None else rmax)
        assert np.array_equal(hist[b], want), (n, b, np.flatnonzero(hist[b] != want)[:8])
    if rmax is None and n > 2:
        assert hist.sum() > 0
    if n > 2:
        assert not np.array_equal(hist[0], hist[1])          # the replicas differ: each row is its own replica's


# ---- 2. ties ---------------------------------------------------------------------------------------------------------
def test_lattice_ties_on_bin_edges_and_half_box(oracle):
    """unjittered 4 x 4 x 4 simple-cubic lattice in L = 4 with rmax = 2, 8 bins: separations exactly on bin edges
    (r / dr an integer) and components with d / L = +-0.5 -- both true-division paths decide"""
    n, L, rmax, nbins = 64, 4.0, 2.0, 8
    p = md_types.init_params(n, L, 0.005, 1.9)
    g = np.arange(4, dtype=np.float64)
    site = np.stack([a.ravel() for a in np.meshgrid(g, g, g, indexing="ij")])             # [3, 64], integers
    r = np.stack([site, site + 0.5])                                                      # corners / cell centres
    with BatchEngine(p, 2) as eng:
        _set(eng, r, np.zeros_like(r))
        eng.rdf_configure(nbins, rmax=rmax)
        eng.rdf_accumulate()
        hist, _ = eng.rdf_read()
        x, y, z = eng.get_state(("r",))["r"]
    for b in range(2):
        want = _oracle_hist(oracle, x[b], y[b], z[b], L, nbins, rmax)
        assert want[4] == 2 * 3 * 64 and want.sum() > want[4]                             # r = 1 sits on the edge of bin 4
        assert np.array_equal(hist[b], want), (b, hist[b], want)
        stateless = np.zeros(nbins, dtype=np.uint64)
        analysis.rdf_histogram(x[b], y[b], z[b], L, nbins, rmax, stateless)
        assert np.array_equal(hist[b], stateless), (b, hist[b], stateless)


# ---- 3. accumulation inside steps(), per-replica handle --------------------------------------------------------------
SWEEP = [(108, 0.80, 21), (500, 0.60, 22), (108, 0.95, 23), (1372, 0.70, 24)]     # (n, rho, seed): four different L
NBINS = 120


def _sweep_cfg():
    return [synthetic.make_config(n, seed=s, rho=rho) for n, rho, s in SWEEP]


def _set_per_replica(eng, cfg):
    eng.set_state(*[[c[1][ax] for c in cfg] for ax in range(3)], *[[c[2][ax] for c in cfg] for ax in range(3)])


def _flat_state(eng):
    st = eng.get_state()
    return [np.concatenate(st[key][ax]) for key in ("r", "ru", "v", "a") for ax in range(3)]


@pytest.fixture(scope="module")
def sweep_reference(oracle):
    """computed once: the oracle histograms of the sweep's positions after steps 10, 20, 30, 40 (a handle stepped
    4 x 10, read back with get_state), and state and scalars of a handle with no g(r) configured"""
    cfg = _sweep_cfg()
    snaps = []
    with BatchEngine.per_replica([c[0] for c in cfg]) as eng:
        _set_per_replica(eng, cfg)
        eng.compute_forces()
        for _ in range(4):
            eng.steps(10, observables=False)
            x, y, z = eng.get_state(("r",))["r"]
            snaps.append(np.stack([_oracle_hist(oracle, x[b], y[b], z[b], c[0].box_length, NBINS,
                                                0.5 * c[0].box_length) for b, c in enumerate(cfg)]))
    plain = {}
    for sample_every in (20, 10):
        with BatchEngine.per_replica([c[0] for c in cfg]) as eng:
            _set_per_replica(eng, cfg)
            eng.compute_forces()
            plain[sample_every] = (eng.steps(40, sample_every), _flat_state(eng))
    return cfg, snaps, plain


@pytest.mark.parametrize("every, sample_every", [(10, 20), (20, 10)])
def test_accumulation_inside_steps(sweep_reference, every, sample_every):
    cfg, snaps, plain = sweep_reference
    with BatchEngine.per_replica([c[0] for c in cfg]) as eng:
        _set_per_replica(eng, cfg)
        eng.compute_forces()
        eng.rdf_configure(NBINS, every=every)
        scalars = eng.steps(40, sample_every)
        hist, count = eng.rdf_read()
        state = _flat_state(eng)
        prof = eng.profile_read()
    assert count == 40 // every
    want = sum(snaps[k] for k in range(every // 10 - 1, 4, every // 10))
    assert np.array_equal(hist, want)
    want_scalars, want_state = plain[sample_every]
    for got, ref in zip(scalars, want_scalars):
        assert got.shape == ref.shape and got.tobytes() == ref.tobytes()
    for got, ref in zip(state, want_state):
        assert got.tobytes() == ref.tobytes()
    assert prof["launches"] >= 3 * (1 + 40 // every), prof       # three kernel classes, each with its g(r) launches


# ---- 4. a replica's counts are its own -------------------------------------------------------------------------------
MIX = [(65, 0.60, 31), (108, 0.80, 32), (500, 0.95, 33), (1025, 0.70, 34), (108, 0.85, 35)]


def _mix_counts(cfg):
    with BatchEngine.per_replica([c[0] for c in cfg]) as eng:
        _set_per_replica(eng, cfg)
        eng.compute_forces()
        eng.rdf_configure(100, every=5)
        eng.steps(10, 5)
        eng.rdf_accumulate()
        hist, count = eng.rdf_read()
    assert count == 3
    return hist


def test_counts_do_not_depend_on_batch_slot_neighbours_or_streams(monkeypatch):
    cfg = [synthetic.make_config(n, seed=s, rho=rho) for n, rho, s in MIX]
    B = len(cfg)
    fwd = _mix_counts(cfg)
    rev = _mix_counts(cfg[::-1])
    for b, c in enumerate(cfg):
        p, r, v = c
        with BatchEngine(p, 1) as eng:
            _set(eng, r[None], v[None])
            eng.compute_forces()
            eng.rdf_configure(100, every=5)
            eng.steps(10, 5)
            eng.rdf_accumulate()
            alone, _ = eng.rdf_read()
        assert alone.sum() > 0
        assert np.array_equal(fwd[b], alone[0]), (b, p.n)
        assert np.array_equal(rev[B - 1 - b], alone[0]), (b, p.n)
    monkeypatch.setenv("LJMD_BATCH_GROUP_STREAMS", "0")
    assert np.array_equal(_mix_counts(cfg), fwd)


# ---- 5. reproducible handles -----------------------------------------------------------------------------------------
def test_reproducible_handle(oracle):
    n, B, nbins = 108, 3, 64
    mode = _lib.PRECISION_FP64_REPRODUCIBLE
    p, r, v = _replicas(n, [41, 42, 43])
    L = p.box_length

    def oracle_now(eng):
        x, y, z = eng.get_state(("r",))["r"]
        return np.stack([_oracle_hist(oracle, x[b], y[b], z[b], L, nbins, 0.5 * L) for b in range(B)])

    with BatchEngine(p, B, precision_mode=mode) as eng:
        _set(eng, r, v)
        eng.rdf_configure(nbins)
        eng.rdf_accumulate()
        hist, count = eng.rdf_read()
        assert count == 1 and np.array_equal(hist, oracle_now(eng))
        eng.compute_forces()
        want = hist.copy()
        for _ in range(3):
            eng.steps(8, observables=False)
            want += oracle_now(eng)
        want_state = [np.asarray(a) for key in ("r", "ru", "v", "a") for a in eng.get_state()[key]]
    with BatchEngine(p, B, precision_mode=mode) as eng:
        _set(eng, r, v)
        eng.rdf_configure(nbins, every=8)
        eng.rdf_accumulate()
        eng.compute_forces()
        eng.steps(24, 12)
        hist, count = eng.rdf_read()
        state = [np.asarray(a) for key in ("r", "ru", "v", "a") for a in eng.get_state()[key]]
    assert count == 4 and np.array_equal(hist, want)
    for got, ref in zip(state, want_state):
        assert got.tobytes() == ref.tobytes()


# ---- 6. sequence and guards ------------------------------------------------------------------------------------------
def _code(call):
    with pytest.raises(LjmdError) as ei:
        call()
    return ei.value.code, ei.value.message


def test_sequence_and_guards():
    n, B = 108, 3
    p, r, v = _replicas(n, [51, 52, 53])
    lib = _lib.load()
    with BatchEngine(p, B) as eng:
        assert lib.ljmd_batch_rdf_accumulate(eng._h) == _lib.LJMD_ERR_STATE          # before configure
        assert lib.ljmd_batch_rdf_read(eng._h, None, None) == _lib.LJMD_ERR_STATE
        assert lib.ljmd_batch_rdf_reset(eng._h) == _lib.LJMD_ERR_STATE
        eng.rdf_configure(50)
        assert _code(eng.rdf_accumulate)[0] == _lib.LJMD_ERR_STATE                   # before set_state
        _set(eng, r, v)
        eng.compute_forces()
        for nbins in (-1, 8193):
            assert _code(lambda: eng.rdf_configure(nbins))[0] == _lib.LJMD_ERR_INVALID_ARG
        assert _code(lambda: eng.rdf_configure(50, every=-1))[0] == _lib.LJMD_ERR_INVALID_ARG
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            code, msg = _code(lambda: eng.rdf_configure(50, rmax=[1.0, 1.0, bad]))
            assert code == _lib.LJMD_ERR_INVALID_ARG and "replica 2" in msg, msg
            assert msg.startswith("ljmd_batch_rdf_configure: replica 2:"), msg
        hist, count = eng.rdf_read()                                                 # the refused calls changed nothing
        assert count == 0 and hist.shape == (B, 50) and not hist.any()

        eng.rdf_accumulate()
        once, count = eng.rdf_read()
        assert count == 1 and once.sum() > 0
        eng.rdf_accumulate()
        twice, count = eng.rdf_read()
        assert count == 2 and np.array_equal(twice, 2 * once)
        again, count = eng.rdf_read()                                                # read clears nothing
        assert count == 2 and np.array_equal(again, twice)
        _set(eng, r[::-1].copy(), v)                                                 # set_state keeps the counts
        kept, count = eng.rdf_read()
        assert count == 2 and np.array_equal(kept, twice)
        eng.rdf_reset()
        zero, count = eng.rdf_read()
        assert count == 0 and not zero.any()
        eng.rdf_accumulate()
        swapped, _ = eng.rdf_read()
        assert np.array_equal(swapped, once[::-1])                                   # rows follow the resident replicas

        eng.rdf_configure(75, every=4)                                               # reconfigure: new shape, zeroed
        fresh, count = eng.rdf_read()
        assert count == 0 and fresh.shape == (B, 75) and not fresh.any()
        eng.compute_forces()
        code, msg = _code(lambda: eng.steps(10, 5))                                  # 10 % 4 != 0: nothing launched
        assert code == _lib.LJMD_ERR_INVALID_ARG and "multiple" in msg
        assert eng.rdf_read()[1] == 0
        eng.steps(8, 4)
        assert eng.rdf_read()[1] == 2
        eng.rdf_configure(0)                                                         # off: today's stepping, no counts
        eng.steps(10, 5)
        assert lib.ljmd_batch_rdf_read(eng._h, None, None) == _lib.LJMD_ERR_STATE
