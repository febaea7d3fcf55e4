"""CPU-only: the engine's resident density modes without a GPU.  tests/rhok_host is a program of its own under ASan and
UBSan that checks itself: the host core (csrc/ljmd_rhok.cpp) on the fake HIP runtime, its launchers carrying out the
kernels' meaning on the host, the returned words against a brute-force sum, every guard's code and message, a full
series, the entries limit, NULL outputs, the range word, reconfigure, off and release while configured.  Here also: the
numpy model (tests/rhok_model.py) against a plain Python loop with exact rationals, its distance from the true cos / sin,
its symmetries, ljmd_rhok_select_modes against a restatement of its rule, the entry points' refusal of a NULL handle,
and analysis.static_structure_factor / intermediate_scattering against their definitions.  The kernels are covered on
the GPU: tests/test_gpu_rhok_resident.py."""
import math
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import rhok_model
from conftest import ROOT
from ljmd_amd import Engine, _lib, analysis

H = float.fromhex


def test_rhok_host_code_under_sanitizers():
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc absent: the program cannot be built")
    here = ROOT / "tests" / "rhok_host"
    subprocess.run(["make", "-C", str(here)], check=True, capture_output=True, timeout=600)
    env = {k: v for k, v in os.environ.items() if not k.startswith("LJMD_")}
    env.update(FAKEHIP_DEVICES="1", ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:exitcode=23",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1:exitcode=24")
    out = subprocess.run([str(here / "rhok_host")], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-6000:])
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error:" not in out.stderr, out.stderr[-6000:]
    assert out.stdout.strip().splitlines()[-1] == "rhok_host: ok" and "FAILED" not in out.stdout


def _rint(x: float) -> float:
    """round half to even of a double (Python's round on a float is exactly that)"""
    return float(round(x)) if math.isfinite(x) and abs(x) < 2.0 ** 52 else x


def _Q(t: float) -> int:
    """RNE(t 2^64) in exact rational arithmetic"""
    x = Fraction(t) * 2 ** 64
    f = x.numerator // x.denominator
    rem = x - f
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and f % 2):
        f += 1
    return f


S = {3: H("-0x1.5555555555555p-3"), 5: H("0x1.1111111111111p-7"), 7: H("-0x1.a01a01a01a01ap-13"), 9: H("0x1.71de3a556c734p-19"),
     11: H("-0x1.ae64567f544e4p-26"), 13: H("0x1.6124613a86d09p-33"), 15: H("-0x1.ae7f3e733b81fp-41")}
Cc = {2: H("-0x1p-1"), 4: H("0x1.5555555555555p-5"), 6: H("-0x1.6c16c16c16c17p-10"), 8: H("0x1.a01a01a01a01ap-16"),
      10: H("-0x1.27e4fb7789f5cp-22"), 12: H("0x1.1eed8eff8d898p-29"), 14: H("-0x1.93974a8c07c9dp-37"), 16: H("0x1.ae7f3e733b81fp-45")}


def _term_plain(x, L, n):
    """the definition for one particle and one mode with Python floats (IEEE doubles, one rounding per operation)"""
    t = []
    for a in range(3):
        ta = x[a] / L
        t.append(ta - _rint(ta))
    phi = (float(n[0]) * t[0] + float(n[1]) * t[1]) + float(n[2]) * t[2]
    f = phi - _rint(phi)
    q = _rint(4.0 * f)
    g = f - 0.25 * q
    th = g * H("0x1.921fb54442d18p+2")
    zz = th * th
    ps = S[15]
    for k in (13, 11, 9, 7, 5, 3):
        ps = ps * zz + S[k]
    s = th + th * (zz * ps)
    pc = Cc[16]
    for k in (14, 12, 10, 8, 6, 4, 2):
        pc = pc * zz + Cc[k]
    c = 1.0 + zz * pc
    return [(c, s), (-s, c), (-c, -s), (s, -c)][int(q) & 3], f, q


def _positions(n, L, seed):
    rng = np.random.default_rng(seed)
    r = rng.uniform(-0.2 * L, 1.2 * L, size=(3, n))
    r[:, 3] += 3.0 * L                          # shifted by whole boxes
    r[:, 4] -= 3.0 * L
    r[1, 5] += 3.0 * L
    r[0, 6] = L / 2                             # exactly half a box
    r[0, 7] = L / 8                             # a tie in rint(4 f) with mode (1, 0, 0)
    r[1:, 7] = 0.0
    return r


MODES = [(0, 0, 0), (1, 0, 0), (-3, 2, 7), (1023, -1023, 1023), (-1, 0, 0), (3, -2, -7), (0, 5, 0), (2, 1, 0)]


def test_model_equals_a_plain_loop():
    n, L = 40, 8.0
    r = _positions(n, L, 17)
    got, flag = rhok_model.words(r, L, MODES)
    assert not flag
    for m, mode in enumerate(MODES):
        re = im = 0
        for j in range(n):
            (C, Sn), _f, _q = _term_plain([float(r[a, j]) for a in range(3)], L, mode)
            re += _Q(C)
            im += _Q(Sn)
        assert got[m] == [re, im], mode
    # the special positions are what they are meant to be
    (_cs, f, q) = _term_plain([float(r[a, 7]) for a in range(3)], L, (1, 0, 0))
    assert f == 0.125 and q == 0.0              # 4 f = 0.5 is a tie: to even, down
    (_cs, f, q) = _term_plain([float(r[a, 6]) for a in range(3)], L, (1, 0, 0))[0:3]
    assert abs(f) == 0.5 and abs(q) == 2.0
    # a coordinate that is not finite: two zeros and the flag, the other particles as before
    r2 = r.copy()
    r2[2, 9] = np.nan
    got2, flag2 = rhok_model.words(r2, L, MODES)
    assert flag2
    rest, _ = rhok_model.words(np.delete(r, 9, axis=1), L, MODES)
    assert got2 == rest
    assert rhok_model.words(r, float("nan"), MODES[:2]) == ([[0, 0], [0, 0]], True)
    # limbs
    for x in (0, 1, -1, 2 ** 64, -2 ** 64, 2 ** 191 - 1, -2 ** 191, -(5 << 131) + 7):
        l = rhok_model.to_limbs(x)
        u = [v & (2 ** 64 - 1) for v in l]
        assert all(-2 ** 63 <= v < 2 ** 63 for v in l) and (l[2] << 128) + (u[1] << 64) + u[0] == x


def test_model_term_is_within_the_derived_bound():
    """|C - cos 2 pi phi*| and |S - sin 2 pi phi*| <= 2 pi 2^-53 sum_a |n_a| (|x_a| / L + 1.5) + 2^-51, phi* the exact
    phase sum_a n_a x_a / L of the doubles x_a and L.  Derivation, in turns, with u = 2^-53 (half an ulp of 1):
      x_a / L is rounded once: an error of at most u |x_a| / L; the subtraction of rint is exact and leaves |t_a| <= 1/2;
      the product n_a t_a carries |n_a| times that error and is rounded once: at most u |n_a t_a| <= u |n_a| / 2 more;
      each of the two sums is rounded once, at most u |partial sum| <= u sum_a |n_a| / 2 each, together u sum_a |n_a|;
    so |phi - phi*| <= u sum_a |n_a| (|x_a| / L + 1/2 + 1), and f = phi - rint(phi), q and g = f - q / 4 are exact.  The
    phase error times 2 pi bounds the error of cos and sin (their slopes are at most 1).  On top of it th = g 2 pi and the
    two polynomials: 4 u = 2^-51 is allowed, 1.4 u was measured.  The true values are evaluated in np.longdouble on the
    exact phase reduced to (-1/2, 1/2] in rational arithmetic."""
    if np.finfo(np.longdouble).nmant < 63:
        pytest.skip("np.longdouble is no wider than double here")
    rng = np.random.default_rng(23)
    L = 68.94
    n = 300
    r = rng.uniform(-0.2 * L, 1.2 * L, size=(3, n))
    modes = [(1, 0, 0), (-3, 2, 7), (1023, 1023, -1023), (1023, -1023, 1023), (0, 0, 511), (40, -17, 3), (0, 0, 0)]
    modes += [tuple(int(v) for v in rng.integers(-1023, 1024, 3)) for _ in range(8)]
    with np.errstate(all="ignore"):
        t = np.stack([rhok_model.turns(r[a], L) for a in range(3)])
        C, Sn = rhok_model.terms(t, np.array(modes))
    two_pi = 2 * np.arccos(np.longdouble(-1))
    worst = 0.0
    for m, mode in enumerate(modes):
        for j in range(n):
            ph = sum(Fraction(mode[a]) * Fraction(float(r[a, j])) / Fraction(L) for a in range(3))
            ph -= round(ph)
            ang = two_pi * (np.longdouble(ph.numerator) / np.longdouble(ph.denominator))
            bound = 2 * math.pi * 2.0 ** -53 * sum(abs(mode[a]) * (abs(float(r[a, j])) / L + 1.5) for a in range(3)) + 2.0 ** -51
            ec, es = abs(float(np.longdouble(C[m, j]) - np.cos(ang))), abs(float(np.longdouble(Sn[m, j]) - np.sin(ang)))
            assert ec <= bound and es <= bound, (mode, j, ec, es, bound)
            worst = max(worst, max(ec, es) / bound)
    print("largest error / bound: %.3f" % worst)


def test_model_symmetries():
    n, L = 40, 8.0
    r = _positions(n, L, 5)
    modes = [(1, 0, 0), (-3, 2, 7), (1023, -1023, 1023), (0, 5, 0), (2, 1, 0), (0, 0, 0)]
    pos, _ = rhok_model.words(r, L, modes)
    neg, _ = rhok_model.words(r, L, [tuple(-v for v in m) for m in modes])
    for p, q in zip(pos, neg):
        assert q == [p[0], -p[1]]
    assert any(p[1] != 0 for p in pos)
    assert pos[-1] == [n << 64, 0]
    d = rhok_model.doubles(pos)
    assert d[-1] == complex(n, 0.0) and d.shape == (len(modes),)
    assert d[0].imag == pos[0][1] / 2 ** 64         # CPython's int / int is one correct rounding


def _select_rule(n2_max, per_shell):
    r = int(math.isqrt(n2_max))
    shells = {}
    for x in range(-r, r + 1):
        for y in range(-r, r + 1):
            for z in range(-r, r + 1):
                n2 = x * x + y * y + z * z
                if 1 <= n2 <= n2_max and (x > 0 or (x == 0 and y > 0) or (x == 0 and y == 0 and z > 0)):
                    shells.setdefault(n2, []).append((x, y, z))
    out = []
    for n2 in sorted(shells):
        s = sorted(shells[n2])
        out += s if len(s) <= per_shell else [s[j * len(s) // per_shell] for j in range(per_shell)]
    return np.array(out, dtype=np.int32)


@pytest.mark.parametrize("n2_max, per_shell", [(1, 8), (27, 1), (27, 8), (100, 4)])
def test_select_modes_against_the_rule(n2_max, per_shell):
    want = _select_rule(n2_max, per_shell)
    got = Engine.rhok_select_modes(n2_max, per_shell)
    assert got.dtype == np.int32 and got.shape == want.shape and (got == want).all()
    lib = _lib.load()
    import ctypes as C
    count = C.c_int32(-1)
    buf = np.full((len(want), 3), 77, dtype=np.int32)
    short = len(want) - 1
    assert lib.ljmd_rhok_select_modes(n2_max, per_shell, short, buf.ctypes.data_as(_lib.c_int32_p), C.byref(count)) == _lib.LJMD_ERR_INVALID_ARG
    assert count.value == len(want) and "ljmd_rhok_select_modes" in _lib.last_error() and str(len(want)) in _lib.last_error()
    assert (buf[short:] == 77).all() and (buf[:short] == want[:short]).all()


def test_entry_points_refuse_a_null_handle():
    lib = _lib.load()
    calls = {
        "ljmd_rhok_configure": lambda: lib.ljmd_rhok_configure(None, 0, None, 10),
        "ljmd_rhok_accumulate": lambda: lib.ljmd_rhok_accumulate(None),
        "ljmd_rhok_read_exact": lambda: lib.ljmd_rhok_read_exact(None, None, None),
        "ljmd_rhok_read": lambda: lib.ljmd_rhok_read(None, None, None),
        "ljmd_rhok_reset": lambda: lib.ljmd_rhok_reset(None),
        "ljmd_rhok_profile_read": lambda: lib.ljmd_rhok_profile_read(None, None),
    }
    for name, call in calls.items():
        assert call() == _lib.LJMD_ERR_INVALID_ARG, name
        assert name in _lib.last_error()
    for name in ("rhok_configure", "rhok_accumulate", "rhok_read", "rhok_read_exact", "rhok_reset", "rhok_profile", "rhok_select_modes"):
        assert callable(getattr(Engine, name))
    header = (ROOT / "include" / "ljmd.h").read_text()
    assert "#define LJMD_RHOK_MAX_MODES %d\n" % _lib.RHOK_MAX_MODES in header and _lib.RHOK_MAX_MODES == 4096
    assert "#define LJMD_RHOK_MAX_INDEX %d " % _lib.RHOK_MAX_INDEX in header and _lib.RHOK_MAX_INDEX == 1023
    assert "#define LJMD_RHOK_MAX_SNAPSHOTS %d\n" % _lib.RHOK_MAX_SNAPSHOTS in header and _lib.RHOK_MAX_SNAPSHOTS == 262144
    assert "#define LJMD_RHOK_MAX_ENTRIES (1 << 24) " in header and _lib.RHOK_MAX_ENTRIES == 1 << 24
    for name in list(calls) + ["ljmd_rhok_select_modes"]:
        assert "int %s(" % name in header, name


def test_static_structure_factor_of_a_lattice_and_of_an_ideal_gas():
    # a perfect FCC lattice of 3^3 cells: Bragg peaks S = N where h, k, l are multiples of 3 and all even or all odd
    cells, a = 3, 2.0
    L = cells * a
    basis = np.array([[0, 0, 0], [0.5, 0.5, 0], [0.5, 0, 0.5], [0, 0.5, 0.5]])
    cell = np.stack([g.ravel() for g in np.meshgrid(*[np.arange(cells)] * 3, indexing="ij")], axis=1)
    r = ((cell[:, None, :] + basis[None, :, :]) * a).reshape(-1, 3).T
    N = r.shape[1]
    assert N == 108
    modes = [(3, 3, 3), (6, 0, 0), (1, 0, 0), (2, 1, 0)]
    w, flag = rhok_model.words(r, L, modes)
    assert not flag
    rho = rhok_model.doubles(w)[None, :]
    k, Sk, err, count = analysis.static_structure_factor(rho, N, modes, L)
    # shells in ascending |n|^2: 1, 5, 27, 36
    assert list(count) == [1, 1, 1, 1] and np.isnan(err).all()
    np.testing.assert_allclose(k, 2 * np.pi * np.sqrt([1.0, 5.0, 27.0, 36.0]) / L, rtol=1e-15)
    assert abs(Sk[2] - N) <= 1e-12 * N and abs(Sk[3] - N) <= 1e-12 * N
    assert abs(Sk[0]) < 1e-20 * N and abs(Sk[1]) < 1e-20 * N
    # 200 snapshots of 500 uniform random positions: S(k) = 1 on every shell
    rng = np.random.default_rng(11)
    n, n_snap, L = 500, 200, 9.0
    modes = Engine.rhok_select_modes(12, 6)
    pos = rng.uniform(0.0, L, size=(n_snap, 3, n))
    phase = 2 * np.pi / L * np.einsum("ma,sap->smp", modes.astype(np.float64), pos)
    rho = np.exp(1j * phase).sum(axis=2)
    k, Sk, err, count = analysis.static_structure_factor(rho, n, modes, L)
    shells = sorted(set(int(v) for v in (modes.astype(np.int64) ** 2).sum(axis=1)))
    assert len(Sk) == len(shells) and count.sum() == len(modes)
    np.testing.assert_allclose(k, 2 * np.pi * np.sqrt(np.array(shells, dtype=float)) / L, rtol=1e-15)
    assert (np.abs(Sk - 1.0) <= 4.0 * err).all(), (Sk, err)
    assert (err > 0).all() and (err < 0.2).all()
    with pytest.raises(ValueError):
        analysis.static_structure_factor(rho[:, :-1], n, modes, L)
    with pytest.raises(ValueError):
        analysis.static_structure_factor(rho, n, modes[:, :2], L)


@pytest.mark.parametrize("n_snap, max_lag, stride", [(50, 10, 1), (37, 36, 3), (2, 1, 1)])
def test_intermediate_scattering_against_the_definition(n_snap, max_lag, stride):
    rng = np.random.default_rng(n_snap)
    n = 64
    modes = np.array([(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, -1), (2, 0, 0), (0, 0, 0)])
    rho = rng.normal(size=(n_snap, len(modes))) + 1j * rng.normal(size=(n_snap, len(modes))) + (0.5 - 0.25j)
    F = analysis.intermediate_scattering(rho, n, modes, max_lag, stride)
    shells = [[6], [0, 1, 2], [3, 4], [5]]                  # |n|^2 = 0, 1, 2, 4
    lags = min(max_lag, n_snap - 1) + 1
    assert F.shape == (len(shells), lags)
    want = np.zeros_like(F)
    origins = list(range(0, n_snap - 1, stride))
    for s, members in enumerate(shells):
        acc, cnt = np.zeros(lags), np.zeros(lags)
        for t0 in origins:
            for lag in range(0, min(max_lag, n_snap - 1 - t0) + 1):
                acc[lag] += float(np.mean([(rho[t0 + lag, m] * np.conj(rho[t0, m])).real for m in members]))
                cnt[lag] += 1
        want[s] = acc / np.maximum(cnt, 1) / n
    # sums of at most 50 x 3 products of O(1) numbers in another order: a few ulp of the largest partial sum
    tol = 64 * np.finfo(float).eps * (np.abs(rho).max() ** 2) * 2 / n
    np.testing.assert_allclose(F, want, rtol=0, atol=tol)
    # F(k, 0) is S(k) over the origins used
    _k, Sk, _e, _c = analysis.static_structure_factor(rho[origins], n, modes, 5.0)
    np.testing.assert_allclose(F[:, 0], Sk, rtol=0, atol=tol)
    with pytest.raises(ValueError):
        analysis.intermediate_scattering(rho[:, :-1], n, modes)
