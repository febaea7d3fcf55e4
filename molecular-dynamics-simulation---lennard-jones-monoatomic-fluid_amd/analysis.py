"""Trajectory analysis on rva.dat snapshots: the host-side mirror of the reference's
`compute_rdf`, `compute_msd_tau_timeorig`, `compute_vacf_tau_timeorig`
(scripts/md_one_run_analysis.py:404-595).  SURVEY.md 8(f) #3.

The O(n^2) pair pass of the RDF runs on the GPU (`ljmd_rdf_histogram`, integer histogram,
bit-exact); with `subsample=True` the reference's sub-sampling (<= 200 snapshots, <= 800
particles, chosen with np.linspace) is applied first, so the result equals the reference's
for the same input; `subsample=False` uses every particle of every snapshot -- the case the
reference cannot afford in numpy.  MSD / VACF: `time_origin_average_gpu` (the O(n_snap^2 n) sums in a HIP kernel) beside
the numpy mirror of the reference's functions (bit-identical to the reference module; the CPU tests' checker).
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import c_double_p


def rdf_histogram(x, y, z, L: float, nbins: int, rmax: float, hist: np.ndarray) -> None:
    """Adds one snapshot's ordered-pair distance counts to hist (uint64[nbins]) on the GPU."""
    arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (x, y, z)]
    assert hist.dtype == np.uint64 and hist.shape == (nbins,) and hist.flags.c_contiguous
    _lib.check(_lib.load().ljmd_rdf_histogram(len(arrs[0]), *[a.ctypes.data_as(c_double_p) for a in arrs],
                                              float(L), int(nbins), float(rmax),
                                              hist.ctypes.data_as(C.POINTER(C.c_uint64))))


def compute_rdf(rx: np.ndarray, ry: np.ndarray, rz: np.ndarray, L: float, nbins: int = 200,
                rmax: float | None = None, subsample: bool = True, histogram=rdf_histogram):
    """-> (r_centers, g_r); arrays rx, ry, rz of shape (n_snap, n), wrapped positions."""
    n_snap, n = rx.shape
    if rmax is None:
        rmax = 0.5 * L
    snap_idx = np.arange(n_snap)
    part_idx = np.arange(n)
    if subsample:
        if n_snap > 200:
            snap_idx = np.linspace(0, n_snap - 1, 200, dtype=int)
        if n > 800:
            part_idx = np.linspace(0, n - 1, 800, dtype=int)
    n_eff = len(part_idx)
    if n_eff < 2:
        raise ValueError("Not enough particles for RDF after subsampling.")
    counts = np.zeros(nbins, dtype=np.uint64)
    for s in snap_idx:
        histogram(rx[s, part_idx], ry[s, part_idx], rz[s, part_idx], L, nbins, rmax, counts)
    return rdf_from_histogram(counts, n_eff, L, nbins, rmax, len(snap_idx))


def rdf_from_histogram(hist, n: int, L: float, nbins: int, rmax: float, n_snapshots: int):
    """-> (r_centers, g_r) from pair-distance counts (2 per unordered pair, summed over n_snapshots snapshots of n
    particles in a box of side L): the reference's normalisation (scripts/md_one_run_analysis.py:586-594).  The counts
    of BatchEngine.rdf_read go in row by row."""
    hist = np.asarray(hist).astype(np.float64)     # each unordered pair contributed 2 (i-j and j-i)
    vol = L ** 3
    rho = n / vol
    r_edges = np.linspace(0.0, rmax, nbins + 1)
    r_centers = 0.5 * (r_edges[:-1] + r_edges[1:])
    shell_vol = (4.0 / 3.0) * math.pi * (r_edges[1:] ** 3 - r_edges[:-1] ** 3)
    norm = n_snapshots * n * rho * shell_vol
    g = np.zeros_like(r_centers)
    mask = norm > 0
    g[mask] = hist[mask] / norm[mask]
    return r_centers, g


def time_origin_average_gpu(kind: int, x, y, z, max_lag=None, origin_stride: int = 1) -> np.ndarray:
    """MSD (kind 0: unwrapped positions) / VACF (kind 1: velocities) on the GPU (`ljmd_time_origin_average`): the
    O(n_snap^2 n) particle means per (origin, lag) in a HIP kernel, the origins added on the host in the reference's order.
    Equal to compute_msd_tau_timeorig / compute_vacf_tau_timeorig below to rounding (numpy's mean is a pairwise sum)."""
    arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (x, y, z)]
    n_snap, n = arrs[0].shape
    if n_snap < 2:
        return compute_msd_tau_timeorig(*arrs) if kind == 0 else compute_vacf_tau_timeorig(*arrs)
    max_lag = n_snap - 1 if max_lag is None else int(min(max_lag, n_snap - 1))
    out = np.empty(max_lag + 1, dtype=np.float64)
    _lib.check(_lib.load().ljmd_time_origin_average(kind, n_snap, n, *[a.ctypes.data_as(c_double_p) for a in arrs], max_lag,
                                                    max(1, int(origin_stride)), out.ctypes.data_as(c_double_p)))
    return out


def _time_origin_average(series, max_lag, origin_stride, term):
    n_snap = series[0].shape[0]
    if max_lag is None:
        max_lag = n_snap - 1
    max_lag = int(min(max_lag, n_snap - 1))
    origin_stride = max(1, int(origin_stride))
    acc = np.zeros(max_lag + 1, dtype=np.float64)
    counts = np.zeros(max_lag + 1, dtype=np.int64)
    for t0 in range(0, n_snap - 1, origin_stride):
        lag = min(max_lag, (n_snap - 1) - t0)
        if lag <= 0:
            continue
        acc[:lag + 1] += term(t0, lag)
        counts[:lag + 1] += 1
    mask = counts > 0
    acc[mask] /= counts[mask]
    return acc


def compute_msd_tau_timeorig(rux, ruy, ruz, max_lag=None, origin_stride: int = 1) -> np.ndarray:
    """MSD(tau) = <|ru(t+tau) - ru(t)|^2> over particles and time origins (md_one_run_analysis.py:404-441)."""
    if rux.shape[0] < 2:
        return np.array([0.0], dtype=np.float64)

    def term(t0, lag):
        dx = rux[t0:t0 + lag + 1, :] - rux[t0, :][None, :]
        dy = ruy[t0:t0 + lag + 1, :] - ruy[t0, :][None, :]
        dz = ruz[t0:t0 + lag + 1, :] - ruz[t0, :][None, :]
        return np.mean(dx * dx + dy * dy + dz * dz, axis=1)

    return _time_origin_average((rux,), max_lag, origin_stride, term)


def compute_vacf_tau_timeorig(vx, vy, vz, max_lag=None, origin_stride: int = 1) -> np.ndarray:
    """VACF(tau) = <v(t) . v(t+tau)> over particles and time origins (md_one_run_analysis.py:444-489)."""
    if vx.shape[0] < 2:
        return np.array([np.mean(vx[0] * vx[0] + vy[0] * vy[0] + vz[0] * vz[0])], dtype=np.float64)

    def term(t0, lag):
        return np.mean(vx[t0:t0 + lag + 1, :] * vx[t0, :][None, :] + vy[t0:t0 + lag + 1, :] * vy[t0, :][None, :]
                       + vz[t0:t0 + lag + 1, :] * vz[t0, :][None, :], axis=1)

    return _time_origin_average((vx,), max_lag, origin_stride, term)


def stress_acf(p, max_lag=None, origin_stride: int = 1):
    """p [n_snap, 6]: a pressure-tensor series in the order xx, yy, zz, xy, xz, yz (Engine.stress_read) -> (shear,
    normal): two autocorrelation functions of max_lag + 1 lags, each a mean over three components.  shear: the
    time-origin average of sigma_xy, sigma_xz, sigma_yz; normal: the same of (sigma_xx - sigma_yy) / 2,
    (sigma_yy - sigma_zz) / 2, (sigma_zz - sigma_xx) / 2.  Formula, origin convention and counts are those of
    compute_vacf_tau_timeorig with the three components as the velocity of one particle."""
    p = np.asarray(p, dtype=np.float64)
    if p.ndim != 2 or p.shape[1] != 6:
        raise ValueError(f"stress_acf: p must have shape (n_snap, 6), got {p.shape}")
    xx, yy, zz, xy, xz, yz = (p[:, c][:, None] for c in range(6))
    shear = compute_vacf_tau_timeorig(xy, xz, yz, max_lag, origin_stride) / 3.0
    normal = compute_vacf_tau_timeorig(0.5 * (xx - yy), 0.5 * (yy - zz), 0.5 * (zz - xx), max_lag, origin_stride) / 3.0
    return shear, normal


def viscosity_green_kubo(acf, dt_sample: float, V: float, T: float) -> np.ndarray:
    """Green-Kubo running shear viscosity eta(tau) = V / T * integral_0^tau acf, the integral by the trapezoid rule on the
    sampling grid (eta[0] = 0); reduced units (k_B = 1)."""
    acf = np.asarray(acf, dtype=np.float64)
    run = np.zeros_like(acf)
    run[1:] = np.cumsum(0.5 * (acf[1:] + acf[:-1]) * dt_sample)
    return (V / T) * run


def heat_flux_acf(j, max_lag=None, origin_stride: int = 1) -> np.ndarray:
    """j [n_snap, 3]: a heat-flux series (Engine.heatflux_read) -> the time-origin average of J(0) . J(tau) / 3 at
    max_lag + 1 lags.  Formula, origin convention and counts are those of compute_vacf_tau_timeorig with the three
    components as the velocity of one particle."""
    j = np.asarray(j, dtype=np.float64)
    if j.ndim != 2 or j.shape[1] != 3:
        raise ValueError(f"heat_flux_acf: j must have shape (n_snap, 3), got {j.shape}")
    jx, jy, jz = (j[:, c][:, None] for c in range(3))
    return compute_vacf_tau_timeorig(jx, jy, jz, max_lag, origin_stride) / 3.0


def heat_flux_acf_ensemble(j, max_lag=None, origin_stride: int = 1):
    """j [n_snap, B, 3]: the heat-flux series of a batch of B identical replicas (BatchEngine.heatflux_read) ->
    (mean[max_lag + 1], stderr[max_lag + 1]): per lag the mean over the replicas of heat_flux_acf(j[:, b]) and its
    standard error, the sample standard deviation (ddof = 1) over sqrt(B); with B = 1 the error is not defined (NaN).
    The replicas are taken as independent runs of one state point: the error falls as 1 / sqrt(B)."""
    j = np.asarray(j, dtype=np.float64)
    if j.ndim != 3 or j.shape[2] != 3 or j.shape[1] < 1:
        raise ValueError(f"heat_flux_acf_ensemble: j must have shape (n_snap, B, 3) with B >= 1, got {j.shape}")
    B = j.shape[1]
    acf = np.stack([heat_flux_acf(j[:, b], max_lag, origin_stride) for b in range(B)])
    mean = acf.mean(axis=0)
    if B < 2:
        return mean, np.full_like(mean, np.nan)
    return mean, acf.std(axis=0, ddof=1) / np.sqrt(B)


def thermal_conductivity_green_kubo(acf, dt_sample: float, V: float, T: float) -> np.ndarray:
    """Green-Kubo running thermal conductivity lambda(tau) = V / T^2 * integral_0^tau acf, the integral by the trapezoid
    rule on the sampling grid (lambda[0] = 0); reduced units (k_B = 1)."""
    acf = np.asarray(acf, dtype=np.float64)
    run = np.zeros_like(acf)
    run[1:] = np.cumsum(0.5 * (acf[1:] + acf[:-1]) * dt_sample)
    return (V / (T * T)) * run


# -- collective density modes (Engine.rhok_read: rho[n_snap, n_modes] complex, modes[n_modes, 3] integer triples) ------
def rhok_shells(modes):
    """modes [n_modes, 3] -> (n2[n_shells], members): the distinct |n|^2 of the list in ascending order and, per shell,
    the indices of its modes in list order."""
    modes = np.asarray(modes)
    if modes.ndim != 2 or modes.shape[1] != 3 or modes.shape[0] < 1:
        raise ValueError(f"density modes: modes must have shape (n_modes, 3) with n_modes >= 1, got {modes.shape}")
    n2 = (modes.astype(np.int64) ** 2).sum(axis=1)
    shells = np.unique(n2)
    return shells, [np.flatnonzero(n2 == s) for s in shells]


def _rhok_series(rho, modes, who: str):
    rho = np.asarray(rho, dtype=np.complex128)
    shells, members = rhok_shells(modes)
    if rho.ndim != 2 or rho.shape[0] < 1 or rho.shape[1] != np.asarray(modes).shape[0]:
        raise ValueError(f"{who}: rho must have shape (n_snap >= 1, n_modes = {np.asarray(modes).shape[0]}), got {rho.shape}")
    return rho, shells, members


def static_structure_factor(rho, n: int, modes, L: float):
    """rho [n_snap, n_modes]: a series of density modes of n particles in a box of side L -> (k, S, stderr, n_modes_of),
    one entry per shell of equal |n|^2 in ascending order: k = 2 pi sqrt(|n|^2) / L, S(k) = <|rho_k|^2> / n over the
    snapshots and the shell's modes, the standard error of that mean over the snapshots (each snapshot's value the mean
    over the shell's modes; sample standard deviation, ddof = 1, over sqrt(n_snap); NaN with one snapshot), and the
    number of modes of the shell."""
    rho, shells, members = _rhok_series(rho, modes, "static_structure_factor")
    if n < 1 or not L > 0.0:
        raise ValueError("static_structure_factor: n >= 1 and L > 0")
    n_snap = rho.shape[0]
    per_snap = np.stack([(rho[:, m].real ** 2 + rho[:, m].imag ** 2).mean(axis=1) / n for m in members], axis=1)
    S = per_snap.mean(axis=0)
    err = per_snap.std(axis=0, ddof=1) / np.sqrt(n_snap) if n_snap > 1 else np.full_like(S, np.nan)
    k = 2.0 * np.pi * np.sqrt(shells.astype(np.float64)) / L
    return k, S, err, np.array([len(m) for m in members], dtype=np.int64)


def intermediate_scattering(rho, n: int, modes, max_lag=None, origin_stride: int = 1) -> np.ndarray:
    """rho [n_snap, n_modes] -> F[n_shells, max_lag + 1]: the coherent intermediate scattering function F(k, tau) =
    <Re rho_k(t0 + tau) rho_k*(t0)> / n over the time origins and the shell's modes, the shells in the order of
    static_structure_factor.  Formula, origin convention and counts are those of compute_vacf_tau_timeorig with the
    shell's modes as the particles and (Re, Im, 0) as the velocity; F(k, 0) is S(k) over the origins used."""
    rho, _shells, members = _rhok_series(rho, modes, "intermediate_scattering")
    if n < 1:
        raise ValueError("intermediate_scattering: n >= 1")
    rows = []
    for m in members:
        re, im = np.ascontiguousarray(rho[:, m].real), np.ascontiguousarray(rho[:, m].imag)
        rows.append(compute_vacf_tau_timeorig(re, im, np.zeros_like(re), max_lag, origin_stride) / n)
    return np.stack(rows)


def _rhok_ensemble(rho, n, L, who: str):
    """-> (rho [n_snap, B, n_modes] complex, n[B], L[B] or None, whether the replicas share one n and one L)"""
    rho = np.asarray(rho, dtype=np.complex128)
    if rho.ndim != 3 or rho.shape[0] < 1 or rho.shape[1] < 1:
        raise ValueError(f"{who}: rho must have shape (n_snap >= 1, B >= 1, n_modes), got {rho.shape}")
    B = rho.shape[1]
    n = np.asarray(n)
    if n.shape not in ((), (B,)) or not np.issubdtype(n.dtype, np.integer):
        raise ValueError(f"{who}: n must be an integer or {B} integers")
    n = np.broadcast_to(n, (B,))
    same = bool(np.all(n == n[0]))
    if L is not None:
        L = np.asarray(L, dtype=np.float64)
        if L.shape not in ((), (B,)):
            raise ValueError(f"{who}: L must be a number or {B} numbers")
        L = np.broadcast_to(L, (B,))
        same = same and bool(np.all(L == L[0]))
    return rho, n, L, same


def _replica_mean(per, same: bool):
    """per [B, ...] -> (mean, stderr) over the replicas: sample standard deviation (ddof = 1) over sqrt(B), NaN with
    B = 1; (None, None) when the replicas are not runs of one state point"""
    if not same:
        return None, None
    mean = per.mean(axis=0)
    if per.shape[0] < 2:
        return mean, np.full_like(mean, np.nan)
    return mean, per.std(axis=0, ddof=1) / np.sqrt(per.shape[0])


def static_structure_factor_ensemble(rho, n, modes, L):
    """rho [n_snap, B, n_modes]: the density modes of a batch of B replicas (BatchEngine.rhok_read), n and L a scalar or
    one value per replica -> (per, mean, stderr).  per[b] = static_structure_factor(rho[:, b], n_b, modes, L_b), the tuple
    (k, S, stderr over the snapshots, n_modes_of) of that function.  For replicas of one n and one L, mean[n_shells] is
    the mean of S over the replicas and stderr[n_shells] its standard error, the sample standard deviation (ddof = 1)
    over sqrt(B) (NaN with B = 1): the replicas are taken as independent runs of one state point, so the error falls as
    1 / sqrt(B).  Otherwise mean and stderr are None (k differs from replica to replica)."""
    rho, n, L, same = _rhok_ensemble(rho, n, L, "static_structure_factor_ensemble")
    per = [static_structure_factor(rho[:, b], int(n[b]), modes, float(L[b])) for b in range(rho.shape[1])]
    mean, err = _replica_mean(np.stack([p[1] for p in per]), same)
    return per, mean, err


def intermediate_scattering_ensemble(rho, n, modes, max_lag=None, origin_stride: int = 1):
    """rho [n_snap, B, n_modes] (BatchEngine.rhok_read), n a scalar or one value per replica -> (per, mean, stderr).
    per[b] = intermediate_scattering(rho[:, b], n_b, modes, max_lag, origin_stride), stacked to [B, n_shells,
    max_lag + 1].  For replicas of one n, mean[n_shells, max_lag + 1] and stderr are the mean over the replicas and its
    standard error as in static_structure_factor_ensemble; otherwise None.  (F is a function of the shell and the lag in
    snapshots: replicas of one n and different L or dt are averaged only if the caller means that.)"""
    rho, n, _L, same = _rhok_ensemble(rho, n, None, "intermediate_scattering_ensemble")
    per = np.stack([intermediate_scattering(rho[:, b], int(n[b]), modes, max_lag, origin_stride) for b in range(rho.shape[1])])
    mean, err = _replica_mean(per, same)
    return per, mean, err


# -- collective current modes (Engine.current_read: j[n_snap, n_modes, 3] complex, modes[n_modes, 3] integer triples) ----
def _current_series(j, n, modes, who: str):
    """-> (j_L [n_snap, n_modes] complex, j_T [n_snap, n_modes, 3] complex, |n|^2 [n_shells], members) with the shell of
    |n|^2 = 0 left out: its direction is undefined.  k^ = n / |n|, j_L = k^ . j, j_T = j - k^ j_L."""
    j = np.asarray(j, dtype=np.complex128)
    shells, members = rhok_shells(modes)
    modes = np.asarray(modes)
    if j.ndim != 3 or j.shape[0] < 1 or j.shape[1] != modes.shape[0] or j.shape[2] != 3:
        raise ValueError(f"{who}: j must have shape (n_snap >= 1, n_modes = {modes.shape[0]}, 3), got {j.shape}")
    if n < 1:
        raise ValueError(f"{who}: n >= 1")
    keep = [i for i, s in enumerate(shells) if s > 0]
    if not keep:
        raise ValueError(f"{who}: no mode with |n|^2 > 0")
    nd = modes.astype(np.float64)
    norm = np.sqrt((nd * nd).sum(axis=1))
    khat = np.zeros_like(nd)
    np.divide(nd, norm[:, None], out=khat, where=norm[:, None] > 0)
    j_L = (j * khat[None, :, :]).sum(axis=2)
    j_T = j - khat[None, :, :] * j_L[:, :, None]
    return j_L, j_T, shells[keep], [members[i] for i in keep]


def _independent_modes(modes, member):
    """the members of a shell grouped so that a mode, its conjugate -n and their duplicates form one group: j_-k = j_k*
    carries nothing that j_k does not"""
    groups = {}
    for m in member:
        t = tuple(int(c) for c in np.asarray(modes)[m])
        neg = tuple(-c for c in t)
        groups.setdefault(max(t, neg), []).append(m)
    return list(groups.values())


def current_equal_time(j, n: int, modes, L: float):
    """j [n_snap, n_modes, 3]: a series of current modes of n particles in a box of side L -> (k, C_L0, C_T0, stderr_L,
    stderr_T, n_modes_of), one entry per shell of equal |n|^2 > 0 in ascending order, the layout of
    static_structure_factor: k = 2 pi sqrt(|n|^2) / L, C_L0 = <|j_L|^2> / n and C_T0 = 1/2 <|j_T|^2> / n over the snapshots
    and the shell's modes (both are the mean square of one Cartesian velocity component in equilibrium), and the
    standard errors of these means: over the snapshots, as static_structure_factor has it, or with ONE snapshot over the
    shell's independent modes, a mode, its conjugate -n and their duplicates counting once (sample standard deviation,
    ddof = 1, over the square root of their number; NaN with fewer than two)."""
    j_L, j_T, shells, members = _current_series(j, n, modes, "current_equal_time")
    if not L > 0.0:
        raise ValueError("current_equal_time: n >= 1 and L > 0")
    n_snap = j_L.shape[0]
    val_L = (j_L.real ** 2 + j_L.imag ** 2) / n                              # [n_snap, n_modes]
    val_T = 0.5 * (j_T.real ** 2 + j_T.imag ** 2).sum(axis=2) / n
    C_L0 = np.array([val_L[:, m].mean(axis=1).mean() for m in members])
    C_T0 = np.array([val_T[:, m].mean(axis=1).mean() for m in members])
    err_L, err_T = np.full_like(C_L0, np.nan), np.full_like(C_T0, np.nan)
    for s, m in enumerate(members):
        if n_snap > 1:
            err_L[s] = val_L[:, m].mean(axis=1).std(ddof=1) / np.sqrt(n_snap)
            err_T[s] = val_T[:, m].mean(axis=1).std(ddof=1) / np.sqrt(n_snap)
            continue
        groups = _independent_modes(modes, m)
        if len(groups) > 1:
            err_L[s] = np.array([val_L[0, g].mean() for g in groups]).std(ddof=1) / np.sqrt(len(groups))
            err_T[s] = np.array([val_T[0, g].mean() for g in groups]).std(ddof=1) / np.sqrt(len(groups))
    k = 2.0 * np.pi * np.sqrt(shells.astype(np.float64)) / L
    return k, C_L0, C_T0, err_L, err_T, np.array([len(m) for m in members], dtype=np.int64)


def current_correlations(j, n: int, modes, L: float, max_lag=None, origin_stride: int = 1):
    """j [n_snap, n_modes, 3] -> (k, C_L[n_shells, max_lag + 1], C_T[n_shells, max_lag + 1]): the longitudinal and
    transverse current correlation functions C_L(k, tau) = <Re j_L(t0 + tau) j_L*(t0)> / n and C_T(k, tau) = 1/2 <Re
    j_T(t0 + tau) . j_T*(t0)> / n over the time origins and the shell's modes, the shells in the order of
    current_equal_time.  Formula, origin convention and counts are those of compute_vacf_tau_timeorig with the shell's
    modes as the particles, as intermediate_scattering has them; at tau = 0 they are current_equal_time over the origins
    used."""
    j_L, j_T, shells, members = _current_series(j, n, modes, "current_correlations")
    if not L > 0.0:
        raise ValueError("current_correlations: n >= 1 and L > 0")
    rows_L, rows_T = [], []
    for m in members:
        re, im = np.ascontiguousarray(j_L[:, m].real), np.ascontiguousarray(j_L[:, m].imag)
        rows_L.append(compute_vacf_tau_timeorig(re, im, np.zeros_like(re), max_lag, origin_stride) / n)
        re = [np.ascontiguousarray(j_T[:, m, a].real) for a in range(3)]
        im = [np.ascontiguousarray(j_T[:, m, a].imag) for a in range(3)]
        rows_T.append(0.5 * (compute_vacf_tau_timeorig(*re, max_lag, origin_stride)
                             + compute_vacf_tau_timeorig(*im, max_lag, origin_stride)) / n)
    k = 2.0 * np.pi * np.sqrt(shells.astype(np.float64)) / L
    return k, np.stack(rows_L), np.stack(rows_T)


def transverse_viscosity(C_T, k, dt_sample: float, number_density: float) -> np.ndarray:
    """C_T [n_shells, n_lags] (current_correlations), k [n_shells] -> eta[n_shells, n_lags]: the running wave-vector
    dependent shear viscosity
        eta(k, t) = rho C_T(k, 0) / (k^2 integral_0^t C_T(k, s) ds),
    rho the number density, the integral the trapezoid running integral on the sampling grid like viscosity_green_kubo's;
    reduced units (m = 1).  For C_T(k, t) = C_T(k, 0) exp(-k^2 eta t / rho), the hydrodynamic form, eta(k, t) -> eta as
    t -> infinity; its k -> 0 limit is the shear viscosity of viscosity_green_kubo.  Where the integral is 0 (t = 0) the
    value is +inf."""
    C_T = np.asarray(C_T, dtype=np.float64)
    k = np.asarray(k, dtype=np.float64)
    if C_T.ndim != 2 or C_T.shape[1] < 1 or k.shape != (C_T.shape[0],):
        raise ValueError(f"transverse_viscosity: C_T must have shape (n_shells, n_lags) and k (n_shells,), got {C_T.shape} "
                         f"and {k.shape}")
    if not dt_sample > 0.0 or not number_density > 0.0 or not np.all(k > 0.0):
        raise ValueError("transverse_viscosity: dt_sample > 0, number_density > 0 and k > 0")
    run = np.zeros_like(C_T)
    run[:, 1:] = np.cumsum(0.5 * (C_T[:, 1:] + C_T[:, :-1]) * dt_sample, axis=1)
    out = np.full_like(C_T, np.inf)
    np.divide(number_density * C_T[:, :1] / (k * k)[:, None], run, out=out, where=run != 0.0)
    return out


# -- van Hove self-correlation (Engine.vanhove_read: hist[max_lag + 1, nbins + 1] with the overflow column last) --------
def _vanhove_rows(hist, counts, n: int):
    """-> (inside [rows, nbins] float64, overflow fraction [rows], 1 / (n count) [rows], 0 where count == 0)"""
    hist = np.asarray(hist)
    counts = np.asarray(counts, dtype=np.float64)
    if hist.ndim != 2 or hist.shape[1] < 2 or counts.shape != (hist.shape[0],) or n < 1:
        raise ValueError("van Hove: hist must be [max_lag + 1, nbins + 1], counts [max_lag + 1], n >= 1")
    norm = np.zeros_like(counts)
    np.divide(1.0, n * counts, out=norm, where=counts > 0)
    return hist[:, :-1].astype(np.float64), hist[:, -1].astype(np.float64) * norm, norm


def van_hove_self(hist, counts, n: int, dr: float):
    """-> (r_centers[nbins], G_s[max_lag + 1, nbins], overflow[max_lag + 1]): G_s[l, b] = H[l, b] / (n count[l]
    V_shell(b)) with V_shell(b) = 4 pi / 3 ((b + 1)^3 - b^3) dr^3, so that sum_b G_s[l, b] V_shell(b) = 1 - overflow[l],
    the fraction of the displacements beyond rmax.  Rows without an origin (count 0) are 0."""
    inside, overflow, norm = _vanhove_rows(hist, counts, n)
    b = np.arange(inside.shape[1], dtype=np.float64)
    shell = 4.0 * math.pi / 3.0 * ((b + 1.0) ** 3 - b ** 3) * dr ** 3
    return (b + 0.5) * dr, inside * norm[:, None] / shell[None, :], overflow


def self_intermediate_scattering(hist, counts, n: int, dr: float, k):
    """-> (F_s, overflow[max_lag + 1]): F_s(k, l) = sum_b H[l, b] sinc(k r_b) / (n count[l]) at the bin centres r_b =
    (b + 1/2) dr, sinc(x) = sin(x) / x -- the isotropic average of exp(i k . d) over the displacements inside rmax.
    k a number -> F_s[max_lag + 1]; k an array -> F_s[k.shape + (max_lag + 1,)].  The displacements in the overflow
    column are left out: their fraction is returned beside it."""
    inside, overflow, norm = _vanhove_rows(hist, counts, n)
    centres = (np.arange(inside.shape[1], dtype=np.float64) + 0.5) * dr
    k = np.asarray(k, dtype=np.float64)
    weight = np.sinc(k[..., None] * centres / math.pi)           # np.sinc(x) = sin(pi x) / (pi x)
    return (weight[..., None, :] * inside).sum(axis=-1) * norm, overflow      # one row's sum does not depend on k's shape


def non_gaussian_parameter(r2, r4):
    """alpha_2 = 3 <r^4> / (5 <r^2>^2) - 1 per lag (0 for a Gaussian distribution of displacements in three dimensions);
    0 where <r^2> == 0"""
    r2 = np.asarray(r2, dtype=np.float64)
    r4 = np.asarray(r4, dtype=np.float64)
    out = np.zeros(np.broadcast(r2, r4).shape)
    np.divide(3.0 * r4, 5.0 * (r2 * r2), out=out, where=r2 != 0.0)
    return np.where(r2 != 0.0, out - 1.0, 0.0)


def van_hove_self_ensemble(hist, counts, n: int, dr: float):
    """hist [B, max_lag + 1, nbins + 1]: the histograms of a batch of B identical replicas (BatchEngine.vanhove_read),
    counts [max_lag + 1] -> (r_centers[nbins], mean[max_lag + 1, nbins], stderr[max_lag + 1, nbins],
    overflow[max_lag + 1]): per (lag, bin) the mean over the replicas of van_hove_self(hist[b], counts, n, dr) and its
    standard error, the sample standard deviation (ddof = 1) over sqrt(B); with B = 1 the error is not defined (NaN).
    overflow is the replica mean of the fraction beyond rmax.  The replicas are taken as independent runs of one state
    point: the error falls as 1 / sqrt(B)."""
    hist = np.asarray(hist)
    if hist.ndim != 3 or hist.shape[0] < 1:
        raise ValueError(f"van_hove_self_ensemble: hist must have shape (B, max_lag + 1, nbins + 1) with B >= 1, got "
                         f"{hist.shape}")
    B = hist.shape[0]
    per = [van_hove_self(hist[b], counts, n, dr) for b in range(B)]
    g = np.stack([p[1] for p in per])
    overflow = np.stack([p[2] for p in per]).mean(axis=0)
    mean = g.mean(axis=0)
    if B < 2:
        return per[0][0], mean, np.full_like(mean, np.nan), overflow
    return per[0][0], mean, g.std(axis=0, ddof=1) / np.sqrt(B), overflow
