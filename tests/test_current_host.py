"""CPU-only: the engine's resident current modes without a GPU.  tests/current_host is a program of its own under ASan
and UBSan that checks itself: the host core (csrc/ljmd_current.cpp) on the fake HIP runtime, its launchers carrying out
the kernels' meaning on the host through csrc/ljmd_current_arith.h, the returned words against a brute-force sum, every
guard's code and message, a full series, the entries limit, NULL outputs, the range word, reconfigure, off and release
while configured.  It prints one system and the words it read; here they are compared with the numpy model
(tests/current_model.py).  Here also: the model's exact consequences, its distance from the true v cos / v sin, its range
rule, the entry points' refusal of a NULL handle, and analysis.current_equal_time / current_correlations /
transverse_viscosity against their definitions.  The kernels are covered on the GPU: tests/test_gpu_current_resident.py."""
import math
import os
import shutil
import subprocess
from decimal import Decimal, getcontext
from fractions import Fraction

import numpy as np
import pytest

import current_model
import rhok_model
from conftest import ROOT
from ljmd_amd import Engine, _lib, analysis, synthetic

MODES = [(0, 0, 0), (1, 0, 0), (-1, 0, 0), (-3, 2, 7), (3, -2, -7), (1023, -1023, 1023), (0, 5, 0), (2, 1, 0), (1, 0, 0)]


def _system(n, L, seed):
    rng = np.random.default_rng(seed)
    r = rng.uniform(-0.2 * L, 1.2 * L, size=(3, n))
    r[:, 3] += 3.0 * L                          # shifted by whole boxes
    r[:, 4] -= 3.0 * L
    r[0, 6] = L / 2                             # exactly half a box
    r[0, 7] = L / 8                             # a tie in rint(4 f) with mode (1, 0, 0)
    r[1:, 7] = 0.0
    v = rng.normal(size=(3, n)) * 1.3
    return r, v


def test_current_host_code_under_sanitizers():
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc absent: the program cannot be built")
    here = ROOT / "tests" / "current_host"
    subprocess.run(["make", "-C", str(here)], check=True, capture_output=True, timeout=600)
    env = {k: v for k, v in os.environ.items() if not k.startswith("LJMD_")}
    env.update(FAKEHIP_DEVICES="1", ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:exitcode=23",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1:exitcode=24")
    out = subprocess.run([str(here / "current_host")], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-6000:])
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error:" not in out.stderr, out.stderr[-6000:]
    lines = out.stdout.strip().splitlines()
    assert lines[-1] == "current_host: ok" and "FAILED" not in out.stdout
    # the system the program printed, through the model
    L = [float.fromhex(l.split()[1]) for l in lines if l.startswith("L ")]
    part = np.array([[float.fromhex(t) for t in l.split()[1:]] for l in lines if l.startswith("particle ")])
    modes = np.array([[int(t) for t in l.split()[1:]] for l in lines if l.startswith("mode ")])
    got = np.array([[int(t) for t in l.split()[1:]] for l in lines if l.startswith("words")], dtype=np.int64)
    assert len(L) == 1 and part.shape == (65, 6) and modes.shape == (9, 3) and got.shape == (9, 18)
    want, flag = current_model.words(part[:, :3].T, part[:, 3:].T, L[0], modes)
    assert not flag
    assert (got.reshape(9, 3, 2, 3) == current_model.to_words(want)).all()


def test_model_consequences():
    """at n = 65 with 9 modes: (1) mode -n is the exact conjugate of mode n; (2) mode (0, 0, 0) is the total momentum
    sum_j Q(v_a) with Im = 0; (3) with every velocity (1, -1, 2) the x words are the density modes' words, the y words
    their negation and the z words twice them -- exactly where no term lies below 2^-12, within one unit per such term
    otherwise."""
    n, L = 65, 8.0
    r, v = _system(n, L, 17)
    w, flag = current_model.words(r, v, L, MODES)
    assert not flag and len(w) == 9
    for a, b in ((1, 2), (3, 4)):
        for c in range(3):
            assert w[a][c][0] == w[b][c][0] and w[a][c][1] == -w[b][c][1]
    assert any(w[3][c][1] != 0 for c in range(3))
    assert w[1] == w[8]                                                         # the duplicate
    for c in range(3):
        total = sum(int(round(Fraction(float(x)) * 2 ** 64)) for x in v[c])     # Python's round of a Fraction is half-even
        assert w[0][c] == [total, 0]
    ones = np.array([[1.0], [-1.0], [2.0]]) * np.ones((1, n))
    wj, flag = current_model.words(r, ones, L, MODES)
    wr, flag_r = rhok_model.words(r, L, MODES)
    assert not flag and not flag_r
    # Q(2 t) = 2 Q(t) where t 2^64 is an integer -- |t| >= 2^-12, or 0; a smaller term's t 2^64 is rounded, and RNE(2 x) is
    # 2 RNE(x) only where x is within 1/4 of an integer: at most one unit per such term
    with np.errstate(all="ignore"):
        CS = rhok_model.terms(np.stack([rhok_model.turns(r[a], L) for a in range(3)]), np.array(MODES))
    small = [((np.abs(t) < 2.0 ** -12) & (t != 0.0)).sum(axis=1) for t in CS]
    for m in range(len(MODES)):
        assert wj[m][0] == wr[m]
        assert wj[m][1] == [-wr[m][0], -wr[m][1]]
        for c in range(2):
            assert abs(wj[m][2][c] - 2 * wr[m][c]) <= small[c][m]
    assert sum(int((s == 0).sum()) for s in small) >= 16                        # exactly twice on nearly every mode
    # the smallest case of the rounding: one particle whose cosine is far below 2^-12
    t = 0.25 * (1 + 2.0 ** -30)
    one_r, two = np.array([[t * L], [0.0], [0.0]]), np.array([[1.0], [-1.0], [2.0]])
    w1, _ = current_model.words(one_r, two, L, [(1, 0, 0)])
    C1 = float(rhok_model.terms(np.stack([rhok_model.turns(one_r[a], L) for a in range(3)]), np.array([(1, 0, 0)]))[0][0, 0])
    assert 0 < abs(C1) < 2.0 ** -12 and w1[0][0][0] == int(round(Fraction(C1) * 2 ** 64))
    assert w1[0][2][0] == int(round(Fraction(2 * C1) * 2 ** 64)) and w1[0][1][0] == -w1[0][0][0]
    d = current_model.doubles(w)
    assert d.shape == (9, 3) and d[0, 1] == complex(w[0][1][0] / 2 ** 64, 0.0)   # CPython's int / int is one correct rounding


PI50 = Decimal("3.14159265358979323846264338327950288419716939937510")


def _cos_sin(x: Decimal):
    """Taylor series of cos and sin at 50 digits, |x| <= pi"""
    c, s, term, k = Decimal(0), Decimal(0), Decimal(1), 0
    while abs(term) > Decimal(10) ** -48 or k < 4:
        if k % 2 == 0:
            c += term if k % 4 == 0 else -term
        else:
            s += term if k % 4 == 1 else -term
        k += 1
        term = term * x / k
    return c, s


def test_model_term_is_within_the_derived_bound():
    """|Q(P_a) 2^-64 - v_a cos 2 pi phi*| and |Q(R_a) 2^-64 - v_a sin 2 pi phi*| <= |v_a| (B + u (1 + B)) + 2^-65 with
    u = 2^-53, phi* the exact phase sum_a n_a x_a / L of the doubles x_a and L, and B = 2 pi u sum_a |n_a| (|x_a| / L +
    1.5) + 2^-51 the documented bound of the density modes' C and S (tests/test_rhok_host.py derives it).  Derivation:
    |C - cos| <= B, so |v_a C - v_a cos| <= |v_a| B; the product is rounded once, at most u |v_a C| <= u |v_a| (1 + B)
    more (a product in the subnormal range is off by at most 2^-1075 instead, far below the last part); Q rounds t 2^64
    to an integer, at most 2^-65 in t.  The true values are evaluated at 50 decimal digits on the exact phase reduced to
    (-1/2, 1/2] in rational arithmetic; the model's terms are taken one particle at a time, so that each word is one
    Q."""
    getcontext().prec = 50
    n, L = 65, 68.94
    r, v = _system(n, L, 23)
    u = 2.0 ** -53
    worst = 0.0
    for j in range(n):
        w, flag = current_model.words(r[:, j:j + 1], v[:, j:j + 1], L, MODES)
        assert not flag
        for m, mode in enumerate(MODES):
            ph = sum(Fraction(mode[a]) * Fraction(float(r[a, j])) / Fraction(L) for a in range(3))
            ph -= round(ph)
            cs = _cos_sin(2 * PI50 * Decimal(ph.numerator) / Decimal(ph.denominator))
            B = 2 * math.pi * u * sum(abs(mode[a]) * (abs(float(r[a, j])) / L + 1.5) for a in range(3)) + 2.0 ** -51
            for a in range(3):
                va = Fraction(float(v[a, j]))
                bound = abs(float(v[a, j])) * (B + u * (1 + B)) + 2.0 ** -65
                for part in range(2):
                    true = Decimal(va.numerator) / Decimal(va.denominator) * cs[part]
                    err = abs(float(Decimal(w[m][a][part]) / Decimal(2 ** 64) - true))
                    assert err <= bound, (mode, j, a, part, err, bound)
                    worst = max(worst, err / bound)
    print("largest error / bound: %.3f" % worst)


def test_model_range_rule():
    """one particle each at v_x = 2^40, v_y = NaN and v_z = inf: the flag is set, and exactly the affected (particle, mode)
    terms are zero in all six sums -- every mode of the NaN and the infinite particle, and of the 2^40 particle the modes
    where |C| or |S| is 1, so that a product reaches the bound."""
    n, L = 65, 8.0
    r, v = _system(n, L, 29)
    r[:, 10] = [0.0, 0.0, 0.0]                  # C = 1 for every mode: v_x C = 2^40
    r[:, 11] = [0.3 * L, 0.1 * L, 0.7 * L]      # ... and a generic place beside it
    clean, flag = current_model.words(r, v, L, MODES)
    assert not flag
    v[0, 10] = v[0, 11] = 2.0 ** 40
    v[1, 20] = np.nan
    v[2, 30] = np.inf
    got, flag = current_model.words(r, v, L, MODES)
    assert flag
    with np.errstate(all="ignore"):
        t = np.stack([rhok_model.turns(r[a], L) for a in range(3)])
        C, S = rhok_model.terms(t, np.array(MODES))
    dropped_any = kept_any = False
    for m, mode in enumerate(MODES):
        gone = [20, 30] + [j for j in (10, 11) if max(abs(C[m, j]), abs(S[m, j])) >= 1.0]
        assert 10 in gone
        dropped_any |= 11 in gone
        kept_any |= 11 not in gone
        keep = [j for j in range(n) if j not in gone]
        want, f = current_model.words(r[:, keep], v[:, keep], L, [mode])
        assert not f and got[m] == want[0], mode
    assert dropped_any and kept_any             # mode (0, 0, 0) has C = 1 everywhere; (-3, 2, 7) has |C|, |S| < 1 there
    # each alone sets the flag
    for (a, j, val) in ((0, 10, 2.0 ** 40), (1, 20, np.nan), (2, 30, -np.inf)):
        _r, vv = _system(n, L, 29)
        vv[a, j] = val
        r2 = r.copy()
        assert current_model.words(r2, vv, L, MODES[:2])[1]
    # just below the bound is in range
    _r, vv = _system(n, L, 29)
    vv[0, 10] = np.nextafter(2.0 ** 40, 0.0)
    assert not current_model.words(r, vv, L, MODES)[1]
    assert clean != got


def test_entry_points_refuse_a_null_handle():
    lib = _lib.load()
    calls = {
        "ljmd_current_configure": lambda: lib.ljmd_current_configure(None, 0, None, 10),
        "ljmd_current_accumulate": lambda: lib.ljmd_current_accumulate(None),
        "ljmd_current_read_exact": lambda: lib.ljmd_current_read_exact(None, None, None),
        "ljmd_current_read": lambda: lib.ljmd_current_read(None, None, None),
        "ljmd_current_reset": lambda: lib.ljmd_current_reset(None),
        "ljmd_current_profile_read": lambda: lib.ljmd_current_profile_read(None, None),
    }
    for name, call in calls.items():
        assert call() == _lib.LJMD_ERR_INVALID_ARG, name
        assert name in _lib.last_error()
    for name in ("current_configure", "current_accumulate", "current_read", "current_read_exact", "current_reset", "current_profile"):
        assert callable(getattr(Engine, name))
    header = (ROOT / "include" / "ljmd.h").read_text()
    assert "#define LJMD_CURRENT_MAX_SNAPSHOTS %d\n" % _lib.CURRENT_MAX_SNAPSHOTS in header and _lib.CURRENT_MAX_SNAPSHOTS == 262144
    assert "#define LJMD_CURRENT_MAX_ENTRIES (1 << 22) " in header and _lib.CURRENT_MAX_ENTRIES == 1 << 22
    for name in calls:
        assert "int %s(" % name in header, name


def _lattice_current():
    """8^3 simple-cubic sites with the transverse velocity wave v = u0 cos(k0 . r), k0 = 2 pi (1, 0, 0) / L, u0 normal to
    k0, and the six modes of the shell |n|^2 = 1 through the model -> (j [1, 6, 3], modes, n, L, u0)"""
    m, a = 8, 1.25
    L = m * a
    g = np.arange(m) * a
    r = np.stack([c.ravel() for c in np.meshgrid(g, g, g, indexing="ij")])
    n = r.shape[1]
    u0 = np.array([0.0, 0.3, -0.2])
    v = u0[:, None] * np.cos(2 * np.pi * r[0] / L)[None, :]
    modes = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)])
    w, flag = current_model.words(r, v, L, modes)
    assert not flag and n == 512
    return current_model.doubles(w)[None, :, :], modes, n, L, u0


def test_current_equal_time_of_a_transverse_wave():
    j, modes, n, L, u0 = _lattice_current()
    # j(+-k0) = sum_j u0 cos^2(k0 x_j) = n u0 / 2 (the imaginary part, sum cos sin, and the other four modes vanish on
    # the lattice), so over the six modes <|j_T|^2> = 2 (n |u0| / 2)^2 / 6 and C_T0 = 1/2 <|j_T|^2> / n = n |u0|^2 / 24
    np.testing.assert_allclose(j[0, 0], n * u0 / 2, rtol=1e-13, atol=1e-11)
    k, CL0, CT0, eL, eT, count = analysis.current_equal_time(j, n, modes, L)
    assert k.shape == CL0.shape == CT0.shape == eL.shape == eT.shape == count.shape == (1,) and count[0] == 6
    assert k[0] == 2 * np.pi / L
    # every term is within 0.36 x 2.2e-15 of its true value (the derived bound at |n| = 1, |x| / L < 1), 512 of them within
    # 4.1e-13, against |j| = 92: 4.5e-15 relative, twice that in the square
    np.testing.assert_allclose(CT0[0], n * (u0 @ u0) / 24, rtol=1e-13)
    assert 0.0 <= CL0[0] < 1e-24                                                 # (3 x 4.1e-13)^2 / 512
    # one snapshot: the error over the three independent modes (k0 with -k0, and the two pairs that vanish)
    per = np.array([n * (u0 @ u0) / 8, 0.0, 0.0])
    np.testing.assert_allclose(eT[0], per.std(ddof=1) / np.sqrt(3), rtol=1e-12)
    assert eL[0] < 1e-24
    # the half-space alone gives the same mean; a shell of one independent mode has no error; |n|^2 = 0 is left out
    k3, CL3, CT3, eL3, eT3, c3 = analysis.current_equal_time(j[:, ::2], n, modes[::2], L)
    np.testing.assert_allclose(CT3, CT0, rtol=1e-14)
    with_zero = np.concatenate([modes[:2], [[0, 0, 0]]])
    k1, _CL1, CT1, _eL1, eT1, c1 = analysis.current_equal_time(j[:, [0, 1, 0]], n, with_zero, L)
    assert k1.shape == (1,) and c1[0] == 2 and np.isnan(eT1[0])
    np.testing.assert_allclose(CT1[0], n * (u0 @ u0) / 8, rtol=1e-13)
    # tau = 0 of the correlation functions
    kc, CL, CT = analysis.current_correlations(j, n, modes, L)
    assert CL.shape == CT.shape == (1, 1) and (kc == k).all()
    np.testing.assert_allclose(CT[:, 0], CT0, rtol=1e-14)
    np.testing.assert_allclose(CL[:, 0], CL0, rtol=1e-12, atol=1e-30)


def test_current_correlations_and_viscosity_of_a_decaying_wave():
    j0, modes, n, L, u0 = _lattice_current()
    gamma, dt, n_snap = 0.7, 0.05, 41
    t = np.arange(n_snap) * dt
    j = j0 * np.exp(-gamma * t)[:, None, None]
    # every origin: tau = 0 is current_equal_time over the origins used (all but the last snapshot)
    k, CL, CT = analysis.current_correlations(j, n, modes, L, max_lag=10, origin_stride=1)
    assert CL.shape == CT.shape == (1, 11)
    _k, CL0, CT0, _eL, eT, _c = analysis.current_equal_time(j[:-1], n, modes, L)
    np.testing.assert_allclose(CT[:, 0], CT0, rtol=1e-13)
    np.testing.assert_allclose(CL[:, 0], CL0, rtol=1e-9, atol=1e-28)
    assert eT[0] > 0                                                             # over the snapshots now
    # the one origin t0 = 0: C_T(tau) = C_T(0) exp(-gamma tau) exactly, C_T(0) = n |u0|^2 / 24
    k, CL, CT = analysis.current_correlations(j, n, modes, L, max_lag=None, origin_stride=n_snap)
    assert CT.shape == (1, n_snap)
    np.testing.assert_allclose(CT[0], n * (u0 @ u0) / 24 * np.exp(-gamma * t), rtol=1e-12)
    assert np.abs(CL).max() < 1e-24
    # eta(k, t_m) = rho C(0) / (k^2 I_m) with the trapezoid integral of the exponential on the grid, q = exp(-gamma dt):
    # I_m = C(0) dt (1 + q) (1 - q^m) / (2 (1 - q)), so eta = rho gamma / k^2 x F_m with the trapezoid factor
    # F_m = 2 (1 - q) / (gamma dt (1 + q) (1 - q^m)) -> 1 for dt -> 0, m dt -> infinity
    rho = n / L ** 3
    eta = analysis.transverse_viscosity(CT, k, dt, rho)
    assert eta.shape == CT.shape and np.isinf(eta[0, 0])
    q = math.exp(-gamma * dt)
    m = np.arange(1, n_snap)
    F = 2 * (1 - q) / (gamma * dt * (1 + q) * (1 - q ** m))
    np.testing.assert_allclose(eta[0, 1:], rho * gamma / k[0] ** 2 * F, rtol=1e-11)
    assert abs(F[-1] * (1 - q ** m[-1]) - 1.0) < 2e-4                            # the factor of the rule itself


def test_analysis_argument_checks():
    j, modes, n, L, _u0 = _lattice_current()
    for f in (analysis.current_equal_time, analysis.current_correlations):
        with pytest.raises(ValueError):
            f(j[:, :-1], n, modes, L)
        with pytest.raises(ValueError):
            f(j[:, :, :2], n, modes, L)
        with pytest.raises(ValueError):
            f(j[0], n, modes, L)
        with pytest.raises(ValueError):
            f(j, n, modes[:, :2], L)
        with pytest.raises(ValueError):
            f(j, 0, modes, L)
        with pytest.raises(ValueError):
            f(j, n, modes, 0.0)
        with pytest.raises(ValueError):
            f(j[:, :1], n, [(0, 0, 0)], L)                                        # no direction
    CT, k = np.ones((2, 5)), np.array([1.0, 2.0])
    for args in ((CT, k[:1], 0.1, 0.8), (CT[0], k, 0.1, 0.8), (CT, k, 0.0, 0.8), (CT, k, 0.1, 0.0), (CT, np.array([0.0, 1.0]), 0.1, 0.8)):
        with pytest.raises(ValueError):
            analysis.transverse_viscosity(*args)


@pytest.mark.parametrize("n", [500, 4096])
def test_equipartition_of_the_model(n):
    """every one of the 61 independent wave vectors with 0 < |n|^2 <= 9 carries <|j_L|^2> / n = 1/2 <|j_T|^2> / n = <v_a^2>:
    the velocities of synthetic.make_config are independent of the positions.  The means over the 122 modes, a mode and
    its conjugate counting once, lie within 4 standard errors of sum v^2 / (3 n); plain numpy gives deviations of 0.3 to
    1.3 standard errors for these inputs, so the bound holds for the definition alone."""
    p, r, v = synthetic.make_config(n, seed=1000 + n, rho=0.8)
    L = p.box_length
    g = np.arange(-3, 4)
    modes = np.array([(x, y, z) for x in g for y in g for z in g if 0 < x * x + y * y + z * z <= 9])
    assert modes.shape == (122, 3)
    w, flag = current_model.words(r, v, L, modes)
    assert not flag
    j = current_model.doubles(w)
    khat = modes / np.sqrt((modes ** 2).sum(axis=1))[:, None]
    jL = (j * khat).sum(axis=1)
    jT = j - khat * jL[:, None]
    vL = np.abs(jL) ** 2 / n
    vT = 0.5 * (np.abs(jT) ** 2).sum(axis=1) / n
    half = np.array([m for m in range(122) if tuple(modes[m]) > tuple(-modes[m])])
    assert half.size == 61
    for m in half:                                                               # the conjugate carries the same value
        o = int(np.flatnonzero((modes == -modes[m]).all(axis=1))[0])
        assert vL[o] == vL[m] and vT[o] == vT[m]
    want = float((np.asarray(v) ** 2).sum() / (3 * n))
    for name, val in (("L", vL[half]), ("T", vT[half])):
        mean, err = val.mean(), val.std(ddof=1) / np.sqrt(half.size)
        print("n = %d  C_%s0 = %.6f +- %.6f  against %.6f: %.2f standard errors" % (n, name, mean, err, want, abs(mean - want) / err))
        assert abs(mean - want) <= 4.0 * err, (name, mean, err, want)
