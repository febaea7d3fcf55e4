"""CPU-only: the host core of the engine's resident pressure tensor (csrc/ljmd_stress.cpp) on the fake HIP runtime.
tests/stress_host is a program of its own under ASan and UBSan that checks itself: its launchers carry out the kernels'
meaning on the host -- boxes, walk, skipping, tie rule, doubling, partials, fold -- and the words the core returns must
equal a brute-force sum over the ordered pairs, on one rank and as rank partials, with every guard's return code and
message, a full series, NULL outputs and the range word.  Here also: ljmd_stress_from_exact against Python ints,
analysis.stress_acf against the brute-force definition, the model against a plain Python loop, and that the entry points
exist and refuse a NULL handle (they are covered on the GPU: tests/test_gpu_stress_resident.py)."""
import math
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import stress_model
from conftest import ROOT
from ljmd_amd import Engine, _lib, analysis
from reproducible_model import R


def test_stress_host_code_under_sanitizers():
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc absent: the program cannot be built")
    here = ROOT / "tests" / "stress_host"
    subprocess.run(["make", "-C", str(here)], check=True, capture_output=True, timeout=600)
    env = {k: v for k, v in os.environ.items() if not k.startswith("LJMD_")}
    env.update(FAKEHIP_DEVICES="1", ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:exitcode=23",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1:exitcode=24")
    out = subprocess.run([str(here / "stress_host")], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-6000:])
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error:" not in out.stderr, out.stderr[-6000:]
    assert out.stdout.strip().splitlines()[-1] == "stress_host: ok" and "FAILED" not in out.stdout


def test_entry_points_refuse_a_null_handle():
    lib = _lib.load()
    calls = {
        "ljmd_stress_configure": lambda: lib.ljmd_stress_configure(None, 10),
        "ljmd_stress_accumulate": lambda: lib.ljmd_stress_accumulate(None),
        "ljmd_stress_read_exact": lambda: lib.ljmd_stress_read_exact(None, None, None),
        "ljmd_stress_read": lambda: lib.ljmd_stress_read(None, None, None),
        "ljmd_stress_reset": lambda: lib.ljmd_stress_reset(None),
        "ljmd_stress_profile_read": lambda: lib.ljmd_stress_profile_read(None, None, None, None),
    }
    for name, call in calls.items():
        assert call() == _lib.LJMD_ERR_INVALID_ARG, name
        assert name in _lib.last_error()
    for name in ("stress_configure", "stress_accumulate", "stress_read", "stress_read_exact", "stress_reset", "stress_profile"):
        assert callable(getattr(Engine, name))
    assert _lib.STRESS_MAX_SNAPSHOTS == 262144
    header = (ROOT / "include" / "ljmd.h").read_text()
    assert "#define LJMD_STRESS_MAX_SNAPSHOTS 262144" in header


def _from_exact(w, L):
    words = np.array([stress_model.to_limbs(x) for x in w], dtype=np.int64)
    out = np.full(6, np.nan)
    assert _lib.load().ljmd_stress_from_exact(words.ctypes.data_as(_lib.c_int64_p), L,
                                              out.ctypes.data_as(_lib.c_double_p)) == _lib.LJMD_OK
    return out


def test_from_exact_is_one_rounding_per_integer():
    tie_even = (2 ** 53 + 1) << 20            # 54 significant bits, the last one set: a tie, rounds to even (down)
    tie_odd = (2 ** 53 + 3) << 20             # ... rounds to even (up)
    ints = [0, 1, -1, 12345678901234567890123, -98765432109876543210987, 3 << 130, -(5 << 131) + 7, (1 << 150) - 1,
            tie_even, -tie_even, tie_odd, tie_even + 1, tie_even - 1, (2 ** 53 + 1) << 100, 2 ** 191 - 1, -2 ** 191]
    assert R(tie_even) == float(2 ** 53 << 20) / 2.0 ** 64 and R(tie_odd) == float((2 ** 53 + 4) << 20) / 2.0 ** 64
    rng = np.random.default_rng(5)
    for L in (17.235477520255067, 4.0, 68.94):
        V = (L * L) * L
        for _ in range(8):
            w = [ints[k] for k in rng.integers(0, len(ints), 12)]
            got = _from_exact(w, L)
            want = np.array([(R(w[c]) + 12.0 * R(w[6 + c])) / V for c in range(6)])
            assert got.tobytes() == want.tobytes(), (w, L, got, want)
            assert got.tobytes() == stress_model.doubles(w, L).tobytes()
    lib = _lib.load()
    out = np.zeros(6)
    words = np.zeros(36, dtype=np.int64)
    assert lib.ljmd_stress_from_exact(None, 1.0, out.ctypes.data_as(_lib.c_double_p)) == _lib.LJMD_ERR_INVALID_ARG
    assert "ljmd_stress_from_exact" in _lib.last_error()
    assert lib.ljmd_stress_from_exact(words.ctypes.data_as(_lib.c_int64_p), 1.0, None) == _lib.LJMD_ERR_INVALID_ARG
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert lib.ljmd_stress_from_exact(words.ctypes.data_as(_lib.c_int64_p), bad,
                                          out.ctypes.data_as(_lib.c_double_p)) == _lib.LJMD_ERR_INVALID_ARG


def test_limbs_round_trip():
    for x in (0, 1, -1, 2 ** 64, -2 ** 64, 2 ** 191 - 1, -2 ** 191, -(5 << 131) + 7):
        l = stress_model.to_limbs(x)
        u = [v & (2 ** 64 - 1) for v in l]
        assert all(-2 ** 63 <= v < 2 ** 63 for v in l)
        assert (l[2] << 128) + (u[1] << 64) + u[0] == x


def test_model_equals_a_plain_loop():
    """the vectorised model against the definition written as a double loop over the ordered pairs with Python floats
    (IEEE doubles, no contraction) and Q(t) = t 2^64 rounded half to even in exact rational arithmetic"""
    rng = np.random.default_rng(17)
    n, L, rc = 40, 4.0, 1.9
    g = np.stack([a.ravel() for a in np.meshgrid(*[np.arange(4.0)] * 3, indexing="ij")])[:, :n]
    r = g + 0.3 * rng.random((3, n))
    r[:, 1] = r[:, 0] + np.array([0.05, 0.0, 0.0])        # one pair out of range
    r[0, 5] += 2 * L                                        # an image two boxes away
    v = rng.normal(size=(3, n))
    v[1, 7] = 2.0 ** 21                                     # vy*vy = 2^42: the particle's six products enter as 0

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

    K, S, flag = [0] * 6, [0] * 6, False
    for i in range(n):
        w = [float(v[k, i]) for k in range(3)]
        t = [w[0] * w[0], w[1] * w[1], w[2] * w[2], w[0] * w[1], w[0] * w[2], w[1] * w[2]]
        if all(abs(x) < 2.0 ** 40 for x in t):
            K = [a + Q(x) for a, x in zip(K, t)]
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
            t = [f[0] * d[0], f[1] * d[1], f[2] * d[2], f[0] * d[1], f[0] * d[2], f[1] * d[2]]
            if all(abs(x) < 2.0 ** 40 for x in t + f + [u6]):
                S = [a + Q(x) for a, x in zip(S, t)]
            else:
                flag = True
    got, gflag = stress_model.words(r, v, L, rc)
    assert flag and gflag
    assert got == K + S
    assert S[0] != 0 and S[3] != 0 and K[3] != 0
    # a rank's partial: its rows only; two halves add up
    a, _ = stress_model.words(r, v, L, rc, rows=np.arange(0, n // 2))
    b, _ = stress_model.words(r, v, L, rc, rows=np.arange(n // 2, n))
    assert [x + y for x, y in zip(a, b)] == got and a != b


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
def test_stress_acf_against_the_definition(n_snap, max_lag, stride):
    rng = np.random.default_rng(n_snap)
    p = rng.normal(size=(n_snap, 6)) + np.array([5.0, 5.0, 5.0, 0.0, 0.0, 0.0])
    shear, normal = analysis.stress_acf(p, max_lag, stride)
    lags = min(max_lag, n_snap - 1) + 1
    assert shear.shape == normal.shape == (lags,)
    want_s = _acf_brute(p[:, 3:6], max_lag, stride)
    nd = 0.5 * np.stack([p[:, 0] - p[:, 1], p[:, 1] - p[:, 2], p[:, 2] - p[:, 0]], axis=1)
    want_n = _acf_brute(nd, max_lag, stride)
    # sums of at most 50 products of O(1) numbers in another order: a few ulp of the largest partial sum
    np.testing.assert_allclose(shear, want_s, rtol=0, atol=64 * np.finfo(float).eps * np.abs(p[:, 3:6]).max() ** 2 * 3)
    np.testing.assert_allclose(normal, want_n, rtol=0, atol=64 * np.finfo(float).eps * np.abs(nd).max() ** 2 * 3)
    with pytest.raises(ValueError):
        analysis.stress_acf(p[:, :5])


def test_viscosity_green_kubo_is_the_running_trapezoid():
    acf = np.array([4.0, 2.0, 1.0, 0.5, 0.0, -0.25])
    eta = analysis.viscosity_green_kubo(acf, 0.1, V=8.0, T=2.0)
    want = (8.0 / 2.0) * np.array([0.0, 0.3, 0.45, 0.525, 0.55, 0.5375])
    np.testing.assert_allclose(eta, want, rtol=1e-15, atol=0)
    assert eta[0] == 0.0
    # a constant integrates to a line
    np.testing.assert_allclose(analysis.viscosity_green_kubo(np.ones(11), 0.5, 3.0, 1.5), 2.0 * 0.5 * np.arange(11), rtol=1e-15)
