"""CPU-only: the host core of the engine's resident heat flux (csrc/ljmd_heatflux.cpp) on the fake HIP runtime.
tests/heatflux_host is a program of its own under ASan and UBSan that checks itself: its launchers carry out the kernels'
meaning on the host -- boxes, walk, skipping, tie rule, doubling, partials, fold -- and the words the core returns must
equal a brute-force sum over the ordered pairs, with every guard's return code and message, the refusal of rank engines
and multi-device views, a full series, NULL outputs and the range word.  Here also: ljmd_heatflux_from_exact against
exact rational arithmetic, analysis.heat_flux_acf against the brute-force definition, the model against a plain Python
loop, and that the entry points exist and refuse a NULL handle (they are covered on the GPU:
tests/test_gpu_heatflux_resident.py)."""
import math
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import heatflux_model
from conftest import ROOT
from ljmd_amd import Engine, _lib, analysis
from reproducible_model import R


def test_heatflux_host_code_under_sanitizers():
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc absent: the program cannot be built")
    here = ROOT / "tests" / "heatflux_host"
    subprocess.run(["make", "-C", str(here)], check=True, capture_output=True, timeout=600)
    env = {k: v for k, v in os.environ.items() if not k.startswith("LJMD_")}
    env.update(FAKEHIP_DEVICES="1", ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:exitcode=23",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1:exitcode=24")
    out = subprocess.run([str(here / "heatflux_host")], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-6000:])
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error:" not in out.stderr, out.stderr[-6000:]
    assert out.stdout.strip().splitlines()[-1] == "heatflux_host: ok" and "FAILED" not in out.stdout


def test_entry_points_refuse_a_null_handle():
    lib = _lib.load()
    calls = {
        "ljmd_heatflux_configure": lambda: lib.ljmd_heatflux_configure(None, 10),
        "ljmd_heatflux_accumulate": lambda: lib.ljmd_heatflux_accumulate(None),
        "ljmd_heatflux_read_exact": lambda: lib.ljmd_heatflux_read_exact(None, None, None),
        "ljmd_heatflux_read": lambda: lib.ljmd_heatflux_read(None, None, None, None),
        "ljmd_heatflux_reset": lambda: lib.ljmd_heatflux_reset(None),
        "ljmd_heatflux_profile_read": lambda: lib.ljmd_heatflux_profile_read(None, None, None, None),
    }
    for name, call in calls.items():
        assert call() == _lib.LJMD_ERR_INVALID_ARG, name
        assert name in _lib.last_error()
    for name in ("heatflux_configure", "heatflux_accumulate", "heatflux_read", "heatflux_read_exact", "heatflux_reset",
                 "heatflux_profile"):
        assert callable(getattr(Engine, name))
    assert _lib.HEATFLUX_MAX_SNAPSHOTS == 262144
    header = (ROOT / "include" / "ljmd.h").read_text()
    assert "#define LJMD_HEATFLUX_MAX_SNAPSHOTS 262144" in header
    for name in list(calls) + ["ljmd_heatflux_from_exact"]:
        assert "int %s(" % name in header, name


def _from_exact(w, L, with_parts=True):
    words = np.array([heatflux_model.to_limbs(x) for x in w], dtype=np.int64)
    j, parts = np.full(3, np.nan), np.full((3, 3), np.nan)
    assert _lib.load().ljmd_heatflux_from_exact(words.ctypes.data_as(_lib.c_int64_p), L, j.ctypes.data_as(_lib.c_double_p),
                                                parts.ctypes.data_as(_lib.c_double_p) if with_parts else None) == _lib.LJMD_OK
    return j, parts


def _rne(x: Fraction) -> float:
    """the double nearest to an exact rational, ties to even (CPython's int / int is correctly rounded)"""
    return x.numerator / x.denominator


def test_from_exact_is_one_rounding_per_integer():
    tie_even = (2 ** 53 + 1) << 20            # 54 significant bits, the last one set: a tie, rounds to even (down)
    tie_odd = (2 ** 53 + 3) << 20             # ... rounds to even (up)
    ints = [0, 1, -1, 12345678901234567890123, -98765432109876543210987, 3 << 130, -(5 << 131) + 7, (1 << 150) - 1,
            tie_even, -tie_even, tie_odd, tie_even + 1, tie_even - 1, (2 ** 53 + 1) << 100, 2 ** 191 - 1, -2 ** 191]
    rng = np.random.default_rng(5)
    for L in (17.235477520255067, 4.0, 68.94):
        V = (L * L) * L
        for _ in range(8):
            w = [ints[k] for k in rng.integers(0, len(ints), 9)]
            j, parts = _from_exact(w, L)
            # exactly one rounding per integer: each R is the rational x / 2^64 rounded once; the doubles that follow
            # are the definition's operations, each rounded once
            r = [_rne(Fraction(x, 1 << 64)) for x in w]
            assert all(r[c] == R(w[c]) for c in range(9))
            want_j = np.array([(0.5 * r[a] + r[3 + a] + 6.0 * r[6 + a]) / V for a in range(3)])
            want_p = np.array([[0.5 * r[a] / V for a in range(3)], [r[3 + a] / V for a in range(3)],
                               [6.0 * r[6 + a] / V for a in range(3)]])
            # 0.5 x is exact; 6 x and the sums round once each: spelled out in rationals for one of them
            a = int(rng.integers(0, 3))
            c6 = _rne(6 * Fraction(r[6 + a]))
            s1 = _rne(Fraction(0.5 * r[a]) + Fraction(r[3 + a]))
            assert want_j[a] == _rne(Fraction(_rne(Fraction(s1) + Fraction(c6))) / Fraction(V))
            assert j.tobytes() == want_j.tobytes(), (w, L, j, want_j)
            assert parts.tobytes() == want_p.tobytes(), (w, L, parts, want_p)
            mj, mp = heatflux_model.doubles(w, L)
            assert j.tobytes() == mj.tobytes() and parts.tobytes() == mp.tobytes()
            assert _from_exact(w, L, with_parts=False)[0].tobytes() == j.tobytes()
    lib = _lib.load()
    out = np.zeros(3)
    words = np.zeros(27, dtype=np.int64)
    assert lib.ljmd_heatflux_from_exact(None, 1.0, out.ctypes.data_as(_lib.c_double_p), None) == _lib.LJMD_ERR_INVALID_ARG
    assert "ljmd_heatflux_from_exact" in _lib.last_error()
    assert lib.ljmd_heatflux_from_exact(words.ctypes.data_as(_lib.c_int64_p), 1.0, None, None) == _lib.LJMD_ERR_INVALID_ARG
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert lib.ljmd_heatflux_from_exact(words.ctypes.data_as(_lib.c_int64_p), bad, out.ctypes.data_as(_lib.c_double_p),
                                            None) == _lib.LJMD_ERR_INVALID_ARG


def test_model_equals_a_plain_loop():
    """the vectorised model against the definition written as a double loop over the ordered pairs of 12 particles with
    Python floats (IEEE doubles, no contraction) and Q(t) = t 2^64 rounded half to even in exact rational arithmetic"""
    rng = np.random.default_rng(17)
    n, L, rc = 12, 3.0, 1.4
    g = np.stack([a.ravel() for a in np.meshgrid(*[np.arange(3.0)] * 3, indexing="ij")])[:, :n]
    r = g + 0.3 * rng.random((3, n))
    r[:, 1] = r[:, 0] + np.array([1e-4, 0.0, 0.0])         # one pair out of range
    r[0, 5] += 2 * L                                        # an image two boxes away
    v = rng.normal(size=(3, n))
    v[1, 7] = 2.0 ** 15                                     # k2 = 2^30, k2 vy = 2^45: the particle's three terms enter as 0
    v[2, 9] = 2.0 ** 41                                     # every pair of particle 9 has wz out of range

    def Q(t):
        x = Fraction(t) * 2 ** 64
        f = x.numerator // x.denominator
        rem = x - f
        if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and f % 2):
            f += 1
        return f

    def rnd(x):                                             # half away from zero; x - trunc(x) is exact
        t = float(math.trunc(x))
        return t + (math.copysign(1.0, x) if abs(x - t) >= 0.5 else 0.0)

    def ok(*ts):
        return all(abs(x) < 2.0 ** 40 for x in ts)          # NaN and inf fail

    E, P, Cc, flag, npairs = [0] * 3, [0] * 3, [0] * 3, False, 0
    for i in range(n):
        w = [float(v[k, i]) for k in range(3)]
        k2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
        t = [k2 * w[0], k2 * w[1], k2 * w[2]]
        if ok(k2, *t):
            E = [a + Q(x) for a, x in zip(E, t)]
        else:
            flag = True
        for j in range(n):
            if j == i:
                continue
            d = []
            for k in range(3):
                d0 = float(r[k, i]) - float(r[k, j])
                d.append(d0 - L * rnd(d0 * (1.0 / L)))
            r2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
            if not r2 < rc * rc:
                continue
            u = 1.0 / r2
            u3 = u * u * u
            u6 = u3 * u3
            m = 2.0 * u6 - u3
            f = [m * dk * u for dk in d]
            ww = [float(v[k, i]) + float(v[k, j]) for k in range(3)]
            phi = u6 - u3
            gg = f[0] * ww[0] + f[1] * ww[1] + f[2] * ww[2]
            tp = [phi * x for x in ww]
            tc = [gg * x for x in d]
            if ok(u6, gg, *(f + ww + tp + tc)):
                P = [a + Q(x) for a, x in zip(P, tp)]
                Cc = [a + Q(x) for a, x in zip(Cc, tc)]
                npairs += 1
            else:
                flag = True
    got, gflag = heatflux_model.words(r, v, L, rc)
    assert flag and gflag
    assert got == E + P + Cc
    assert all(x != 0 for x in got)
    _s, _f, stats = heatflux_model.pair_words(r, v, L, rc)
    assert stats["pairs"] == npairs > 0
    # both orders of a pair give the same six terms: the sums are even
    assert all(x % 2 == 0 for x in P + Cc)
    kw, kflag = heatflux_model.kinetic_words(v)
    assert kflag and kw == E


def test_limbs_round_trip():
    for x in (0, 1, -1, 2 ** 64, -2 ** 64, 2 ** 191 - 1, -2 ** 191, -(5 << 131) + 7):
        l = heatflux_model.to_limbs(x)
        u = [v & (2 ** 64 - 1) for v in l]
        assert all(-2 ** 63 <= v < 2 ** 63 for v in l)
        assert (l[2] << 128) + (u[1] << 64) + u[0] == x


def _acf_brute(series, max_lag, stride):
    """<sum_c s_c(t0) s_c(t0 + lag)> / 3 over the origins t0 = 0, stride, ... < n_snap - 1, each origin contributing the lags
    0 .. min(max_lag, n_snap - 1 - t0) (the convention of compute_vacf_tau_timeorig)"""
    n_snap = series.shape[0]
    max_lag = min(max_lag, n_snap - 1)
    acc, cnt = np.zeros(max_lag + 1), np.zeros(max_lag + 1)
    for t0 in range(0, n_snap - 1, stride):
        for lag in range(0, min(max_lag, n_snap - 1 - t0) + 1):
            acc[lag] += float(np.dot(series[t0], series[t0 + lag]))
            cnt[lag] += 1
    return acc / np.maximum(cnt, 1) / 3.0


@pytest.mark.parametrize("n_snap, max_lag, stride", [(50, 10, 1), (37, 36, 3), (20, 100, 2), (2, 1, 1)])
def test_heat_flux_acf_against_the_definition(n_snap, max_lag, stride):
    rng = np.random.default_rng(n_snap)
    j = rng.normal(size=(n_snap, 3)) + np.array([0.5, 0.0, -0.25])
    acf = analysis.heat_flux_acf(j, max_lag, stride)
    lags = min(max_lag, n_snap - 1) + 1
    assert acf.shape == (lags,)
    want = _acf_brute(j, max_lag, stride)
    # sums of at most 50 products of O(1) numbers in another order: a few ulp of the largest partial sum
    np.testing.assert_allclose(acf, want, rtol=0, atol=64 * np.finfo(float).eps * np.abs(j).max() ** 2 * 3)
    assert acf[0] > 0.0
    for bad in (j[:, :2], j[:, 0], np.zeros((4, 6))):
        with pytest.raises(ValueError):
            analysis.heat_flux_acf(bad)


def test_thermal_conductivity_green_kubo_is_the_running_trapezoid():
    acf = np.array([4.0, 2.0, 1.0, 0.5, 0.0, -0.25])
    lam = analysis.thermal_conductivity_green_kubo(acf, 0.1, V=8.0, T=2.0)
    want = (8.0 / 4.0) * np.array([0.0, 0.3, 0.45, 0.525, 0.55, 0.5375])
    np.testing.assert_allclose(lam, want, rtol=1e-15, atol=0)
    assert lam[0] == 0.0
    # a constant integrates to a line
    np.testing.assert_allclose(analysis.thermal_conductivity_green_kubo(np.ones(11), 0.5, 3.0, 1.5),
                               (3.0 / 2.25) * 0.5 * np.arange(11), rtol=1e-15)
