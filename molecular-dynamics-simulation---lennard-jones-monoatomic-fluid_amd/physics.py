"""The reference's operator interface for the hot path, served by the HIP library.

  compute_lj_potential_energy(params, state)   scripts/physics/lj_potential_energy.f90:46
  verlet_step(params, state)                   scripts/physics/verlet.f90:41
  minimum_image / wrap_positions               scripts/physics/geometry_pbc.f90:80,39 (host helpers)

Both operators keep the reference's argument meaning: `state` is updated in place,
the scalar outputs are returned as a tuple in the reference's argument order.  They
go through the *stateless* C entry points (ljmd_compute_lj_potential_energy /
ljmd_verlet_step), i.e. exactly what the Fortran shim modules bind.

`Engine` is the resident-state interface (ljmd_create ... ljmd_verlet_steps): state
stays in HBM between calls and only the per-step scalars come back.  `BatchEngine`
(ljmd_batch_*) steps many independent small replicas of one system at once.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import LjmdError, c_double_p
from .md_types import SimParams, SimState


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(c_double_p)


def _check_array(a, n: int, name: str) -> np.ndarray:
    if a is None:
        raise ValueError(f"{name} is not allocated")
    if not isinstance(a, np.ndarray) or a.dtype != np.float64 or a.ndim != 1 or a.shape[0] != n \
            or not a.flags.c_contiguous:
        raise ValueError(f"{name} must be a contiguous float64 array of length {n}")
    return a


def _guard_force_params(p: SimParams, routine: str) -> None:
    # lj_potential_energy.f90:77-81
    if p.n <= 0:
        raise ValueError(f"{routine}(): params%n must be > 0.")
    if p.box_length <= 0.0:
        raise ValueError(f"{routine}(): params%box_length must be > 0.")
    if p.volume <= 0.0:
        raise ValueError(f"{routine}(): params%volume must be > 0.")
    if p.rc <= 0.0:
        raise ValueError(f"{routine}(): params%rc must be > 0.")
    if p.rc_square <= 0.0:
        raise ValueError(f"{routine}(): params%rc_square must be > 0.")


def compute_lj_potential_energy(params: SimParams, state: SimState):
    """-> (epot, d_epot, dd_epot); overwrites state.ax/ay/az."""
    _guard_force_params(params, "compute_lj_potential_energy")
    if not state.allocated():
        raise ValueError("compute_lj_potential_energy(): state arrays are not allocated.")
    n = params.n
    arrs = [_check_array(getattr(state, k), n, k) for k in ("rx", "ry", "rz", "ax", "ay", "az")]
    e, d, dd = C.c_double(), C.c_double(), C.c_double()
    lib = _lib.load()
    _lib.check(lib.ljmd_compute_lj_potential_energy(
        n, params.box_length, params.rc, *[_ptr(a) for a in arrs],
        C.byref(e), C.byref(d), C.byref(dd)))
    return e.value, d.value, dd.value


def verlet_step(params: SimParams, state: SimState):
    """-> (epot, ekin, d_epot, dd_epot); updates all nine state arrays in place."""
    if params.n <= 0:
        raise ValueError("verlet_step(): params%n must be > 0.")
    if not state.allocated():
        raise ValueError("verlet_step(): state arrays are not allocated.")
    n = params.n
    arrs = [_check_array(getattr(state, k), n, k) for k in SimState.FIELDS]
    out = [C.c_double() for _ in range(4)]
    lib = _lib.load()
    _lib.check(lib.ljmd_verlet_step(n, params.box_length, params.dt, params.rc,
                                    *[_ptr(a) for a in arrs], *[C.byref(o) for o in out]))
    return tuple(o.value for o in out)


def stateless_reset() -> None:
    """Frees the cached engine behind compute_lj_potential_energy / verlet_step (ljmd_stateless_reset)."""
    _lib.load().ljmd_stateless_reset()


def minimum_image(dx: float, box_length: float, inv_box_length: float) -> float:
    """geometry_pbc.f90:80-88 (dnint = round half away from zero); host helper."""
    t = dx * inv_box_length
    n = np.copysign(np.floor(np.abs(t) + 0.5), t)
    return dx - box_length * n


class Engine:
    """HBM-resident simulation on one GPU (or one shard of a multi-GPU run).
    devices=[d0, d1, ...]: ONE process driving several devices (ljmd_create_multi): rank g of len(devices) runs on
    devices[g]; the handle then takes and returns global arrays like a single-GPU one."""

    def __init__(self, params: SimParams, device: int = 0, rank: int = 0, n_ranks: int = 1,
                 precision_mode: int = _lib.PRECISION_FP64, devices=None):
        self._lib = _lib.load()
        self.params = params
        self.rank, self.n_ranks = rank, n_ranks
        self.precision_mode = precision_mode
        h = C.c_void_p()
        if devices is not None:
            devs = (C.c_int32 * len(devices))(*devices)
            _lib.check(self._lib.ljmd_create_multi(C.byref(h), params.n, params.box_length, params.dt, params.rc,
                                                   precision_mode, len(devices), devs))
            self.rank, self.n_ranks = 0, 1          # global arrays in, global arrays out
        else:
            _lib.check(self._lib.ljmd_create(C.byref(h), params.n, params.box_length, params.dt, params.rc,
                                             precision_mode, device, rank, n_ranks))
        self._h = h
        self.shard = params.n // self.n_ranks

    # -- lifecycle ---------------------------------------------------------
    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.ljmd_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _ck(self, status: int) -> None:
        _lib.check(status, self._h)

    # -- state transfer ----------------------------------------------------
    def set_state(self, rx, ry, rz, vx, vy, vz) -> None:
        n = self.params.n
        arrs = [_check_array(np.ascontiguousarray(a, dtype=np.float64), n, "state array")
                for a in (rx, ry, rz, vx, vy, vz)]
        self._ck(self._lib.ljmd_set_state(self._h, *[_ptr(a) for a in arrs]))

    def set_accel(self, ax, ay, az) -> None:
        n = self.params.n
        arrs = [_check_array(np.ascontiguousarray(a, dtype=np.float64), n, "accel array") for a in (ax, ay, az)]
        self._ck(self._lib.ljmd_set_accel(self._h, *[_ptr(a) for a in arrs]))

    def set_unwrapped(self, ux, uy, uz) -> None:
        n = self.params.n
        arrs = [_check_array(np.ascontiguousarray(a, dtype=np.float64), n, "unwrapped array") for a in (ux, uy, uz)]
        self._ck(self._lib.ljmd_set_unwrapped(self._h, *[_ptr(a) for a in arrs]))

    def get_state(self, which=("r", "ru", "v", "a")) -> dict:
        """-> {'r': (x,y,z), 'ru': ..., 'v': ..., 'a': ...} of the owned shard."""
        S = self.shard
        out, ptrs = {}, []
        for key in ("r", "ru", "v", "a"):
            if key in which:
                arrs = tuple(np.empty(S, dtype=np.float64) for _ in range(3))
                out[key] = arrs
                ptrs += [_ptr(a) for a in arrs]
            else:
                ptrs += [None, None, None]
        self._ck(self._lib.ljmd_get_state(self._h, *ptrs))
        return out

    # -- hot path ----------------------------------------------------------
    def compute_forces(self):
        e, d, dd = C.c_double(), C.c_double(), C.c_double()
        self._ck(self._lib.ljmd_compute_forces(self._h, C.byref(e), C.byref(d), C.byref(dd)))
        return e.value, d.value, dd.value

    def verlet_steps(self, nsteps: int):
        """-> (epot[nsteps], ekin[nsteps], d_epot[nsteps], dd_epot[nsteps])"""
        outs = [np.empty(nsteps, dtype=np.float64) for _ in range(4)]
        self._ck(self._lib.ljmd_verlet_steps(self._h, nsteps, *[_ptr(o) for o in outs]))
        return tuple(outs)

    def advance(self, nsteps: int) -> None:
        """nsteps Verlet steps whose observables nobody reads (ljmd_verlet_steps with NULL outputs, as the warm-up of
        the initial-configuration driver): forces-only pair kernel, same trajectory bit for bit"""
        self._ck(self._lib.ljmd_verlet_steps(self._h, nsteps, None, None, None, None))

    # -- asynchronous production loop (snapshot I/O overlapped with the next steps) --------
    def enqueue_steps(self, nsteps: int, sampled: bool = False) -> None:
        """sampled: only the last of the nsteps evaluates epot, d_epot, dd_epot (the step the reference samples,
        md_simulation_program.f90:361); collect_steps returns NaN for the others.  r, v, a, ekin are unchanged."""
        fn = self._lib.ljmd_enqueue_steps_sampled if sampled else self._lib.ljmd_enqueue_steps
        self._ck(fn(self._h, nsteps))

    def migrations(self) -> int:
        """ownership migrations so far (multi-device handle: also the automatic ones, LJMD_MULTI_MIGRATE_EVERY)"""
        return int(self._lib.ljmd_multi_migrations(self._h))

    # -- ownership migration (multi-GPU; include/ljmd.h: ljmd_migrate) ------------------------
    def migrate(self) -> None:
        """deal the particles out to the ranks again by position, on the devices, collectives included (multi-device
        handle, or a rank engine with an RCCL communicator: every rank calls it at the same step)"""
        self._ck(self._lib.ljmd_migrate(self._h))

    def migrate_pack(self) -> None:
        self._ck(self._lib.ljmd_migrate_pack(self._h))

    def migrate_buffer(self):
        """-> (device address, total doubles, own offset, own count) of the migration buffer"""
        tot, off, cnt = C.c_int64(), C.c_int64(), C.c_int64()
        p = self._lib.ljmd_migrate_buffer(self._h, C.byref(tot), C.byref(off), C.byref(cnt))
        return p, tot.value, off.value, cnt.value

    def migrate_deal(self) -> None:
        self._ck(self._lib.ljmd_migrate_deal(self._h))

    def particle_ids(self) -> np.ndarray:
        """ids[j] = index, in the arrays given to set_state, of the particle at position j of this engine's arrays"""
        n = self.shard if self.n_ranks > 1 else self.params.n
        ids = np.empty(n, dtype=np.int32)
        self._ck(self._lib.ljmd_particle_ids(self._h, ids.ctypes.data_as(_lib.c_int32_p)))
        return ids

    def set_observables(self, on: bool) -> None:
        """phase API (sharded engines): forces-only force evaluations while off"""
        self._ck(self._lib.ljmd_set_observables(self._h, 1 if on else 0))

    def collect_steps(self, nsteps: int):
        outs = [np.empty(nsteps, dtype=np.float64) for _ in range(4)]
        self._ck(self._lib.ljmd_collect_steps(self._h, nsteps, *[_ptr(o) for o in outs]))
        return tuple(outs)

    def snapshot_begin(self) -> None:
        self._ck(self._lib.ljmd_snapshot_begin(self._h))

    def snapshot_end(self) -> dict:
        """-> {'r': (x,y,z), 'ru': ..., 'v': ..., 'a': ...} as of the matching snapshot_begin."""
        out = {key: tuple(np.empty(self.shard, dtype=np.float64) for _ in range(3)) for key in ("r", "ru", "v", "a")}
        ptrs = [_ptr(a) for key in ("r", "ru", "v", "a") for a in out[key]]
        self._ck(self._lib.ljmd_snapshot_end(self._h, *ptrs))
        return out

    def kinetic_energy(self) -> float:
        k = C.c_double()
        self._ck(self._lib.ljmd_kinetic_energy(self._h, C.byref(k)))
        return k.value

    # -- split phase (multi-GPU) ---------------------------------------------
    def shard_range(self):
        i0, i1 = C.c_int32(), C.c_int32()
        self._ck(self._lib.ljmd_shard_range(self._h, C.byref(i0), C.byref(i1)))
        return i0.value, i1.value

    def exchange_buffer(self):
        """-> (device address, total doubles, own offset, own count)"""
        tot, off, cnt = C.c_int64(), C.c_int64(), C.c_int64()
        p = self._lib.ljmd_exchange_buffer(self._h, C.byref(tot), C.byref(off), C.byref(cnt))
        return p, tot.value, off.value, cnt.value

    def device_ptr(self, which: int, axis: int) -> int:
        return self._lib.ljmd_device_ptr(self._h, which, axis)

    def stream(self) -> int:
        return self._lib.ljmd_stream(self._h)

    @staticmethod
    def comm_unique_id() -> bytes:
        buf = C.create_string_buffer(_lib.COMM_ID_BYTES)
        _lib.check(_lib.load().ljmd_comm_unique_id(buf))
        return buf.raw

    def comm_init(self, unique_id: bytes) -> None:
        assert len(unique_id) == _lib.COMM_ID_BYTES
        self._ck(self._lib.ljmd_comm_init(self._h, unique_id))

    def comm_size(self) -> int:
        """Ranks in the engine's RCCL communicator as RCCL reports them (0 = none)."""
        return int(self._lib.ljmd_comm_size(self._h))

    def allgather_positions(self) -> None:
        self._ck(self._lib.ljmd_allgather_positions(self._h))

    def memcpy(self, dst: int, src: int, nbytes: int, kind: int) -> None:
        """kind 1 = host->device, 2 = device->host, 3 = device->device (raw addresses)."""
        self._ck(self._lib.ljmd_memcpy(self._h, dst, src, nbytes, kind))

    def synchronize(self) -> None:
        self._ck(self._lib.ljmd_synchronize(self._h))

    def step_begin(self) -> None:
        self._ck(self._lib.ljmd_step_begin(self._h))

    def step_finish(self) -> None:
        self._ck(self._lib.ljmd_step_finish(self._h))

    def step_forces(self) -> None:
        self._ck(self._lib.ljmd_step_forces(self._h))

    def force_buffers(self, external: bool):
        """-> (fpart address, doubles, frecv address, doubles); see include/ljmd.h"""
        fp, fr = C.c_void_p(), C.c_void_p()
        nfp, nfr = C.c_int64(), C.c_int64()
        self._ck(self._lib.ljmd_force_buffers(self._h, 1 if external else 0, C.byref(fp), C.byref(nfp),
                                              C.byref(fr), C.byref(nfr)))
        return fp.value, nfp.value, fr.value, nfr.value

    def forces_partial(self) -> None:
        self._ck(self._lib.ljmd_forces_partial(self._h))

    def read_partials(self, nsteps: int) -> np.ndarray:
        out = np.empty((nsteps, _lib.PARTIAL_STRIDE), dtype=np.float64)
        self._ck(self._lib.ljmd_read_partials(self._h, nsteps, _ptr(out)))
        return out

    def combine_scalars(self, partials_by_rank: np.ndarray):
        """partials_by_rank: [n_ranks, PARTIAL_STRIDE] of ONE step -> (epot, ekin, d_epot, dd_epot)"""
        p = np.ascontiguousarray(partials_by_rank, dtype=np.float64)
        outs = [C.c_double() for _ in range(4)]
        self._ck(self._lib.ljmd_combine_scalars(self._h, _ptr(p), p.shape[0], *[C.byref(o) for o in outs]))
        return tuple(o.value for o in outs)

    @property
    def reproducible(self) -> bool:
        return self.precision_mode == _lib.PRECISION_FP64_REPRODUCIBLE

    def read_partials_exact(self, nsteps: int) -> np.ndarray:
        """Reproducible mode: [nsteps, EXACT_PARTIAL_WORDS] int64 records (ljmd.h: LJMD_EXACT_PARTIAL_WORDS)."""
        out = np.empty((nsteps, _lib.EXACT_PARTIAL_WORDS), dtype=np.int64)
        self._ck(self._lib.ljmd_read_partials_exact(self._h, nsteps, out.ctypes.data_as(_lib.c_int64_p)))
        return out

    def combine_scalars_exact(self, words_by_rank: np.ndarray):
        """words_by_rank: [n_ranks, EXACT_PARTIAL_WORDS] int64 of ONE step -> (epot, ekin, d_epot, dd_epot)"""
        p = np.ascontiguousarray(words_by_rank, dtype=np.int64)
        outs = [C.c_double() for _ in range(4)]
        self._ck(self._lib.ljmd_combine_scalars_exact(self._h, p.ctypes.data_as(_lib.c_int64_p), p.shape[0],
                                                      *[C.byref(o) for o in outs]))
        return tuple(o.value for o in outs)

    def set_tail_corrections(self, on: bool) -> None:
        """the reference's compile-time switch use_tail_corrections (lj_potential_energy.f90:36): off = epot, d_epot,
        dd_epot without the three mean-field tail constants"""
        self._ck(self._lib.ljmd_set_tail_corrections(self._h, 1 if on else 0))

    # -- g(r) of the resident system (include/ljmd.h: ljmd_rdf_*) ---------------------------
    def rdf_configure(self, nbins: int, rmax=None) -> None:
        """ljmd_rdf_configure: nbins bins up to rmax (None = half the box); nbins = 0 switches the feature off.  The
        counts start at zero."""
        r = 0.5 * self.params.box_length if rmax is None else float(rmax)
        self._ck(self._lib.ljmd_rdf_configure(self._h, int(nbins), r))
        self._rdf_nbins = int(nbins)

    def rdf_accumulate(self) -> None:
        """adds the histogram of the positions resident now (stream-ordered: no host wait)"""
        self._ck(self._lib.ljmd_rdf_accumulate(self._h))

    def rdf_read(self):
        """-> (hist[nbins] uint64: 2 per unordered pair with r < rmax, the number of snapshots accumulated); a rank
        engine (n_ranks > 1) returns its partial histogram: 1 per ordered pair (own i, any j)"""
        nbins = getattr(self, "_rdf_nbins", 0)
        hist = np.zeros(max(nbins, 1), dtype=np.uint64)
        count = C.c_int64()
        self._ck(self._lib.ljmd_rdf_read(self._h, hist.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(count)))
        return hist[:nbins], count.value

    def rdf_reset(self) -> None:
        self._ck(self._lib.ljmd_rdf_reset(self._h))

    def rdf_profile(self) -> dict:
        """ljmd_rdf_profile_read for the most recent rdf_accumulate -> {'tile_pairs_visited', 'tile_pairs_total',
        'kernel_ms'}"""
        vis, tot, ms = C.c_int64(), C.c_int64(), C.c_double()
        self._ck(self._lib.ljmd_rdf_profile_read(self._h, C.byref(vis), C.byref(tot), C.byref(ms)))
        return {"tile_pairs_visited": vis.value, "tile_pairs_total": tot.value, "kernel_ms": ms.value}

    # -- MSD / VACF of the resident system (include/ljmd.h: ljmd_tcf_*) --------------------
    def tcf_configure(self, max_lag: int, origin_stride: int = 1) -> None:
        """ljmd_tcf_configure: time-origin averaged MSD(tau) and VACF(tau) up to lag max_lag (in snapshots), every
        origin_stride-th snapshot an origin; max_lag = 0 switches the feature off.  Zeroes the sums.  One-rank engines
        only."""
        for name, val in (("max_lag", max_lag), ("origin_stride", origin_stride)):
            if isinstance(val, bool) or not isinstance(val, (int, np.integer)):
                raise TypeError(f"tcf_configure: {name} must be an integer, got {val!r}")
        self._ck(self._lib.ljmd_tcf_configure(self._h, int(max_lag), int(origin_stride)))
        self._tcf_max_lag = int(max_lag)

    def tcf_accumulate(self) -> None:
        """takes the resident ru and v as the next snapshot (stream-ordered: no host wait)"""
        self._ck(self._lib.ljmd_tcf_accumulate(self._h))

    def _tcf_rows(self, who: str) -> int:
        max_lag = getattr(self, "_tcf_max_lag", 0)
        if max_lag < 1:
            raise ValueError(f"{who}: call tcf_configure with max_lag >= 1 first")
        return max_lag + 1

    def tcf_read(self):
        """-> (msd[max_lag + 1], vacf[max_lag + 1], counts[max_lag + 1] int64, n_snapshots); nothing is cleared"""
        rows = self._tcf_rows("tcf_read")
        msd = np.empty(rows, dtype=np.float64)
        vacf = np.empty(rows, dtype=np.float64)
        counts = np.empty(rows, dtype=np.int64)
        snaps = C.c_int64()
        self._ck(self._lib.ljmd_tcf_read(self._h, msd.ctypes.data_as(c_double_p), vacf.ctypes.data_as(c_double_p),
                                         counts.ctypes.data_as(_lib.c_int64_p), C.byref(snaps)))
        return msd, vacf, counts, snaps.value

    def tcf_read_exact(self, raw: bool = False):
        """-> (sums, counts, n_snapshots): the exact integer sums of Q(term) = RNE(term 2^64), sums[kind, lag] with kind
        0 = MSD, 1 = VACF, as Python ints in an object array -- or, raw=True, the library's int64 words
        [2, max_lag + 1, 3] (three little-endian limbs of a signed 192-bit integer)"""
        rows = self._tcf_rows("tcf_read_exact")
        words = np.empty((2, rows, 3), dtype=np.int64)
        counts = np.empty(rows, dtype=np.int64)
        snaps = C.c_int64()
        self._ck(self._lib.ljmd_tcf_read_exact(self._h, words.ctypes.data_as(_lib.c_int64_p),
                                               counts.ctypes.data_as(_lib.c_int64_p), C.byref(snaps)))
        if raw:
            return words, counts, snaps.value
        u = words.view(np.uint64)
        sums = np.empty(words.shape[:2], dtype=object)
        for idx in np.ndindex(*sums.shape):
            sums[idx] = (int(words[idx][2]) << 128) + (int(u[idx][1]) << 64) + int(u[idx][0])
        return sums, counts, snaps.value

    def tcf_reset(self) -> None:
        self._ck(self._lib.ljmd_tcf_reset(self._h))

    def tcf_profile(self) -> dict:
        """ljmd_tcf_profile_read for the most recent tcf_accumulate -> {'kernel_ms', 'origins_live'}"""
        ms, live = C.c_double(), C.c_int32()
        self._ck(self._lib.ljmd_tcf_profile_read(self._h, C.byref(ms), C.byref(live)))
        return {"kernel_ms": ms.value, "origins_live": live.value}

    # -- van Hove self-correlation of the resident system (include/ljmd.h: ljmd_vanhove_*) ----
    def vanhove_configure(self, max_lag: int, origin_stride: int = 1, nbins: int = 128, rmax=None) -> None:
        """ljmd_vanhove_configure: the distribution G_s(r, tau) of the displacements behind the MSD, up to lag max_lag
        (in snapshots), every origin_stride-th snapshot an origin, nbins bins up to rmax (None = half the box) and an
        overflow column; max_lag = 0 switches the feature off.  Zeroes everything.  One-rank engines only."""
        for name, val in (("max_lag", max_lag), ("origin_stride", origin_stride), ("nbins", nbins)):
            if isinstance(val, bool) or not isinstance(val, (int, np.integer)):
                raise TypeError(f"vanhove_configure: {name} must be an integer, got {val!r}")
        if rmax is not None and (isinstance(rmax, bool) or not isinstance(rmax, (int, float, np.integer, np.floating))):
            raise TypeError(f"vanhove_configure: rmax must be a number, got {rmax!r}")
        r = 0.5 * self.params.box_length if rmax is None else float(rmax)
        self._ck(self._lib.ljmd_vanhove_configure(self._h, int(max_lag), int(origin_stride), int(nbins), r))
        self._vanhove_shape = (int(max_lag), int(nbins))

    def vanhove_accumulate(self) -> None:
        """takes the resident ru as the next snapshot (stream-ordered: no host wait)"""
        self._ck(self._lib.ljmd_vanhove_accumulate(self._h))

    def _vanhove_rows(self, who: str):
        max_lag, nbins = getattr(self, "_vanhove_shape", (0, 0))
        if max_lag < 1:
            raise ValueError(f"{who}: call vanhove_configure with max_lag >= 1 first")
        return max_lag + 1, nbins + 1

    def vanhove_read(self):
        """-> (hist[max_lag + 1, nbins + 1] uint64 with the overflow column last, r2[max_lag + 1], r4[max_lag + 1],
        counts[max_lag + 1] int64, n_snapshots); nothing is cleared"""
        rows, cols = self._vanhove_rows("vanhove_read")
        hist = np.empty((rows, cols), dtype=np.uint64)
        r2 = np.empty(rows, dtype=np.float64)
        r4 = np.empty(rows, dtype=np.float64)
        counts = np.empty(rows, dtype=np.int64)
        snaps = C.c_int64()
        self._ck(self._lib.ljmd_vanhove_read(self._h, hist.ctypes.data_as(C.POINTER(C.c_uint64)), r2.ctypes.data_as(c_double_p),
                                             r4.ctypes.data_as(c_double_p), counts.ctypes.data_as(_lib.c_int64_p),
                                             C.byref(snaps)))
        return hist, r2, r4, counts, snaps.value

    def vanhove_read_exact(self, raw: bool = False):
        """-> (hist, sums, counts, n_snapshots): the counts and the exact integer sums of Q(t) = RNE(t 2^64), sums[kind,
        lag] with kind 0 = r^2, 1 = r^4, as Python ints in an object array -- or, raw=True, the library's int64 words
        [2, max_lag + 1, 3] (three little-endian limbs of a signed 192-bit integer)"""
        rows, cols = self._vanhove_rows("vanhove_read_exact")
        hist = np.empty((rows, cols), dtype=np.uint64)
        words = np.empty((2, rows, 3), dtype=np.int64)
        counts = np.empty(rows, dtype=np.int64)
        snaps = C.c_int64()
        self._ck(self._lib.ljmd_vanhove_read_exact(self._h, hist.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                   words.ctypes.data_as(_lib.c_int64_p),
                                                   counts.ctypes.data_as(_lib.c_int64_p), C.byref(snaps)))
        if raw:
            return hist, words, counts, snaps.value
        u = words.view(np.uint64)
        sums = np.empty(words.shape[:2], dtype=object)
        for idx in np.ndindex(*sums.shape):
            sums[idx] = (int(words[idx][2]) << 128) + (int(u[idx][1]) << 64) + int(u[idx][0])
        return hist, sums, counts, snaps.value

    def vanhove_reset(self) -> None:
        self._ck(self._lib.ljmd_vanhove_reset(self._h))

    def vanhove_profile(self) -> dict:
        """ljmd_vanhove_profile_read for the most recent vanhove_accumulate -> {'kernel_ms', 'origins_live'}"""
        ms, live = C.c_double(), C.c_int32()
        self._ck(self._lib.ljmd_vanhove_profile_read(self._h, C.byref(ms), C.byref(live)))
        return {"kernel_ms": ms.value, "origins_live": live.value}

    # -- pressure tensor of the resident system (include/ljmd.h: ljmd_stress_*) ---------------
    def stress_configure(self, max_snapshots: int) -> None:
        """ljmd_stress_configure: room for max_snapshots snapshots of the pressure tensor on the device; 0 switches the
        feature off.  The series starts empty."""
        if isinstance(max_snapshots, bool) or not isinstance(max_snapshots, (int, np.integer)):
            raise TypeError(f"stress_configure: max_snapshots must be an integer, got {max_snapshots!r}")
        self._ck(self._lib.ljmd_stress_configure(self._h, int(max_snapshots)))
        self._stress_max = int(max_snapshots)

    def stress_accumulate(self) -> None:
        """appends the pressure tensor of the state resident now to the series (stream-ordered: no host wait)"""
        self._ck(self._lib.ljmd_stress_accumulate(self._h))

    def _stress_count(self) -> int:
        """snapshots in the series (ljmd_stress_read_exact without a buffer); raises as the reads do"""
        snaps = C.c_int64()
        self._ck(self._lib.ljmd_stress_read_exact(self._h, None, C.byref(snaps)))
        return snaps.value

    def stress_read(self) -> np.ndarray:
        """-> p[n_snapshots, 6]: xx, yy, zz, xy, xz, yz of (sum v v + 12 sum f d) / V per snapshot, without tail
        correction; nothing is cleared.  Refused on a rank engine (n_ranks > 1), which holds a partial sum."""
        p = np.empty((max(self._stress_count(), 1), 6), dtype=np.float64)
        snaps = C.c_int64()
        self._ck(self._lib.ljmd_stress_read(self._h, p.ctypes.data_as(c_double_p), C.byref(snaps)))
        return p[:snaps.value].copy()

    def stress_read_exact(self, raw: bool = False):
        """-> sums[n_snapshots, 12]: the exact integer sums of Q(term) = RNE(term 2^64), K[6] then S[6], as Python ints
        in an object array -- or, raw=True, the library's int64 words [n_snapshots, 12, 3] (three little-endian limbs
        of a signed 192-bit integer).  A rank engine returns its partial."""
        words = np.empty((max(self._stress_count(), 1), 12, 3), dtype=np.int64)
        snaps = C.c_int64()
        self._ck(self._lib.ljmd_stress_read_exact(self._h, words.ctypes.data_as(_lib.c_int64_p), C.byref(snaps)))
        words = words[:snaps.value].copy()
        if raw:
            return words
        u = words.view(np.uint64)
        sums = np.empty(words.shape[:2], dtype=object)
        for idx in np.ndindex(*sums.shape):
            sums[idx] = (int(words[idx][2]) << 128) + (int(u[idx][1]) << 64) + int(u[idx][0])
        return sums

    def stress_reset(self) -> None:
        self._ck(self._lib.ljmd_stress_reset(self._h))

    def stress_profile(self) -> dict:
        """ljmd_stress_profile_read for the most recent stress_accumulate -> {'tile_pairs_visited',
        'tile_pairs_total', 'kernel_ms'}"""
        vis, tot, ms = C.c_int64(), C.c_int64(), C.c_double()
        self._ck(self._lib.ljmd_stress_profile_read(self._h, C.byref(vis), C.byref(tot), C.byref(ms)))
        return {"tile_pairs_visited": vis.value, "tile_pairs_total": tot.value, "kernel_ms": ms.value}

    # -- heat flux of the resident system (include/ljmd.h: ljmd_heatflux_*) -------------------
    def heatflux_configure(self, max_snapshots: int) -> None:
        """ljmd_heatflux_configure: room for max_snapshots snapshots of the heat flux on the device; 0 switches the
        feature off.  The series starts empty.  One-rank engines only."""
        if isinstance(max_snapshots, bool) or not isinstance(max_snapshots, (int, np.integer)):
            raise TypeError(f"heatflux_configure: max_snapshots must be an integer, got {max_snapshots!r}")
        self._ck(self._lib.ljmd_heatflux_configure(self._h, int(max_snapshots)))

    def heatflux_accumulate(self) -> None:
        """appends the heat flux of the state resident now to the series (stream-ordered: no host wait)"""
        self._ck(self._lib.ljmd_heatflux_accumulate(self._h))

    def _heatflux_count(self) -> int:
        """snapshots in the series (ljmd_heatflux_read_exact without a buffer); raises as the reads do"""
        snaps = C.c_int64()
        self._ck(self._lib.ljmd_heatflux_read_exact(self._h, None, C.byref(snaps)))
        return snaps.value

    def heatflux_read(self):
        """-> (j[n_snapshots, 3], parts[n_snapshots, 3, 3]): the heat flux (1/2 sum v^2 v + sum phi w + 6 sum (f . w) d)
        / V per snapshot and its three summands over V, parts[:, 0] convective, parts[:, 1] potential, parts[:, 2]
        collisional; nothing is cleared."""
        n = max(self._heatflux_count(), 1)
        j = np.empty((n, 3), dtype=np.float64)
        parts = np.empty((n, 3, 3), dtype=np.float64)
        snaps = C.c_int64()
        self._ck(self._lib.ljmd_heatflux_read(self._h, j.ctypes.data_as(c_double_p), parts.ctypes.data_as(c_double_p),
                                              C.byref(snaps)))
        return j[:snaps.value].copy(), parts[:snaps.value].copy()

    def heatflux_read_exact(self, raw: bool = False):
        """-> sums[n_snapshots, 9]: the exact integer sums of Q(term) = RNE(term 2^64), E[3], P[3] then C[3], as Python
        ints in an object array -- or, raw=True, the library's int64 words [n_snapshots, 9, 3] (three little-endian
        limbs of a signed 192-bit integer)."""
        words = np.empty((max(self._heatflux_count(), 1), 9, 3), dtype=np.int64)
        snaps = C.c_int64()
        self._ck(self._lib.ljmd_heatflux_read_exact(self._h, words.ctypes.data_as(_lib.c_int64_p), C.byref(snaps)))
        words = words[:snaps.value].copy()
        if raw:
            return words
        u = words.view(np.uint64)
        sums = np.empty(words.shape[:2], dtype=object)
        for idx in np.ndindex(*sums.shape):
            sums[idx] = (int(words[idx][2]) << 128) + (int(u[idx][1]) << 64) + int(u[idx][0])
        return sums

    def heatflux_reset(self) -> None:
        self._ck(self._lib.ljmd_heatflux_reset(self._h))

    def heatflux_profile(self) -> dict:
        """ljmd_heatflux_profile_read for the most recent heatflux_accumulate -> {'tile_pairs_visited',
        'tile_pairs_total', 'kernel_ms'}"""
        vis, tot, ms = C.c_int64(), C.c_int64(), C.c_double()
        self._ck(self._lib.ljmd_heatflux_profile_read(self._h, C.byref(vis), C.byref(tot), C.byref(ms)))
        return {"tile_pairs_visited": vis.value, "tile_pairs_total": tot.value, "kernel_ms": ms.value}

    # -- density modes of the resident system (include/ljmd.h: ljmd_rhok_*) -------------------
    @staticmethod
    def rhok_select_modes(n2_max: int, per_shell: int) -> np.ndarray:
        """ljmd_rhok_select_modes -> modes[n_modes, 3] (int32): the half-space triples with 1 <= |n|^2 <= n2_max by
        shell, at most per_shell of each shell, evenly spaced in lexicographic order.  Host code: needs no engine."""
        lib = _lib.load()
        count = C.c_int32()
        rc = lib.ljmd_rhok_select_modes(int(n2_max), int(per_shell), 0, None, C.byref(count))
        if rc != _lib.LJMD_OK and count.value <= 0:
            _lib.check(rc)
        modes = np.empty((max(count.value, 1), 3), dtype=np.int32)
        _lib.check(lib.ljmd_rhok_select_modes(int(n2_max), int(per_shell), count.value,
                                              modes.ctypes.data_as(_lib.c_int32_p), C.byref(count)))
        return modes[:count.value].copy()

    def rhok_configure(self, modes, max_snapshots: int) -> None:
        """ljmd_rhok_configure: the mode list (integer triples [n_modes, 3], k = 2 pi n / L) and room for max_snapshots
        snapshots of rho_k on the device; max_snapshots = 0 switches the feature off.  The series starts empty.
        One-rank engines only."""
        if isinstance(max_snapshots, bool) or not isinstance(max_snapshots, (int, np.integer)):
            raise TypeError(f"rhok_configure: max_snapshots must be an integer, got {max_snapshots!r}")
        m = np.asarray(modes if modes is not None else np.zeros((0, 3)))
        if m.size and not np.issubdtype(m.dtype, np.integer):
            raise TypeError("rhok_configure: modes must be integers")
        if m.ndim != 2 or m.shape[1] != 3:
            raise ValueError(f"rhok_configure: modes must have shape [n_modes, 3], got {m.shape}")
        if m.size and np.abs(m).max() > np.iinfo(np.int32).max:
            raise ValueError("rhok_configure: modes must lie within the int32 range")
        m = np.ascontiguousarray(m, dtype=np.int32)
        self._ck(self._lib.ljmd_rhok_configure(self._h, m.shape[0], m.ctypes.data_as(_lib.c_int32_p) if m.size else None,
                                               int(max_snapshots)))
        self._rhok_modes = m.shape[0] if int(max_snapshots) > 0 else 0

    def rhok_accumulate(self) -> None:
        """appends rho_k of the positions resident now to the series (stream-ordered: no host wait)"""
        self._ck(self._lib.ljmd_rhok_accumulate(self._h))

    def _rhok_count(self) -> int:
        """snapshots in the series (ljmd_rhok_read_exact without a buffer); raises as the reads do"""
        snaps = C.c_int64()
        self._ck(self._lib.ljmd_rhok_read_exact(self._h, None, C.byref(snaps)))
        return snaps.value

    def rhok_read(self) -> np.ndarray:
        """-> rho[n_snapshots, n_modes] complex: sum_j (cos k.r_j + i sin k.r_j), each part one rounding of its exact
        integer; nothing is cleared."""
        n, m = max(self._rhok_count(), 1), max(getattr(self, "_rhok_modes", 0), 1)
        rho = np.empty((n, m, 2), dtype=np.float64)
        snaps = C.c_int64()
        self._ck(self._lib.ljmd_rhok_read(self._h, rho.ctypes.data_as(c_double_p), C.byref(snaps)))
        return rho[:snaps.value].copy().view(np.complex128)[..., 0]

    def rhok_read_exact(self, raw: bool = False):
        """-> sums[n_snapshots, n_modes, 2]: the exact integer sums of Q(cos) and Q(sin), Q(t) = RNE(t 2^64), as Python
        ints in an object array -- or, raw=True, the library's int64 words [n_snapshots, n_modes, 2, 3] (three
        little-endian limbs of a signed 192-bit integer)."""
        m = max(getattr(self, "_rhok_modes", 0), 1)
        words = np.empty((max(self._rhok_count(), 1), m, 2, 3), dtype=np.int64)
        snaps = C.c_int64()
        self._ck(self._lib.ljmd_rhok_read_exact(self._h, words.ctypes.data_as(_lib.c_int64_p), C.byref(snaps)))
        words = words[:snaps.value].copy()
        if raw:
            return words
        u = words.view(np.uint64)
        sums = np.empty(words.shape[:3], dtype=object)
        for idx in np.ndindex(*sums.shape):
            sums[idx] = (int(words[idx][2]) << 128) + (int(u[idx][1]) << 64) + int(u[idx][0])
        return sums

    def rhok_reset(self) -> None:
        self._ck(self._lib.ljmd_rhok_reset(self._h))

    def rhok_profile(self) -> dict:
        """ljmd_rhok_profile_read for the most recent rhok_accumulate -> {'kernel_ms'}"""
        ms = C.c_double()
        self._ck(self._lib.ljmd_rhok_profile_read(self._h, C.byref(ms)))
        return {"kernel_ms": ms.value}

    # -- current modes of the resident system (include/ljmd.h: ljmd_current_*) -----------------
    def current_configure(self, modes, max_snapshots: int) -> None:
        """ljmd_current_configure: the mode list (integer triples [n_modes, 3], k = 2 pi n / L; rhok_select_modes gives
        the drivers' list) and room for max_snapshots snapshots of j_k on the device; max_snapshots = 0 switches the
        feature off.  The series starts empty.  One-rank engines only; independent of rhok_configure."""
        if isinstance(max_snapshots, bool) or not isinstance(max_snapshots, (int, np.integer)):
            raise TypeError(f"current_configure: max_snapshots must be an integer, got {max_snapshots!r}")
        m = np.asarray(modes if modes is not None else np.zeros((0, 3)))
        if m.size and not np.issubdtype(m.dtype, np.integer):
            raise TypeError("current_configure: modes must be integers")
        if m.ndim != 2 or m.shape[1] != 3:
            raise ValueError(f"current_configure: modes must have shape [n_modes, 3], got {m.shape}")
        if m.size and np.abs(m).max() > np.iinfo(np.int32).max:
            raise ValueError("current_configure: modes must lie within the int32 range")
        m = np.ascontiguousarray(m, dtype=np.int32)
        self._ck(self._lib.ljmd_current_configure(self._h, m.shape[0], m.ctypes.data_as(_lib.c_int32_p) if m.size else None,
                                                  int(max_snapshots)))
        self._current_modes = m.shape[0] if int(max_snapshots) > 0 else 0

    def current_accumulate(self) -> None:
        """appends j_k of the positions and velocities resident now to the series (stream-ordered: no host wait)"""
        self._ck(self._lib.ljmd_current_accumulate(self._h))

    def _current_count(self) -> int:
        """snapshots in the series (ljmd_current_read_exact without a buffer); raises as the reads do"""
        snaps = C.c_int64()
        self._ck(self._lib.ljmd_current_read_exact(self._h, None, C.byref(snaps)))
        return snaps.value

    def current_read(self) -> np.ndarray:
        """-> j[n_snapshots, n_modes, 3] complex: sum_j v_a (cos k.r_j + i sin k.r_j) for a = x, y, z, each part one
        rounding of its exact integer; nothing is cleared."""
        n, m = max(self._current_count(), 1), max(getattr(self, "_current_modes", 0), 1)
        j = np.empty((n, m, 3, 2), dtype=np.float64)
        snaps = C.c_int64()
        self._ck(self._lib.ljmd_current_read(self._h, j.ctypes.data_as(c_double_p), C.byref(snaps)))
        return j[:snaps.value].copy().view(np.complex128)[..., 0]

    def current_read_exact(self, raw: bool = False):
        """-> sums[n_snapshots, n_modes, 3, 2]: the exact integer sums of Q(v_a cos) and Q(v_a sin), Q(t) = RNE(t 2^64),
        as Python ints in an object array -- or, raw=True, the library's int64 words [n_snapshots, n_modes, 3, 2, 3]
        (three little-endian limbs of a signed 192-bit integer)."""
        m = max(getattr(self, "_current_modes", 0), 1)
        words = np.empty((max(self._current_count(), 1), m, 3, 2, 3), dtype=np.int64)
        snaps = C.c_int64()
        self._ck(self._lib.ljmd_current_read_exact(self._h, words.ctypes.data_as(_lib.c_int64_p), C.byref(snaps)))
        words = words[:snaps.value].copy()
        if raw:
            return words
        u = words.view(np.uint64)
        sums = np.empty(words.shape[:4], dtype=object)
        for idx in np.ndindex(*sums.shape):
            sums[idx] = (int(words[idx][2]) << 128) + (int(u[idx][1]) << 64) + int(u[idx][0])
        return sums

    def current_reset(self) -> None:
        self._ck(self._lib.ljmd_current_reset(self._h))

    def current_profile(self) -> dict:
        """ljmd_current_profile_read for the most recent current_accumulate -> {'kernel_ms'}"""
        ms = C.c_double()
        self._ck(self._lib.ljmd_current_profile_read(self._h, C.byref(ms)))
        return {"kernel_ms": ms.value}

    # -- measurement -----------------------------------------------------------
    def profile_enable(self, on: bool = True) -> None:
        self._ck(self._lib.ljmd_profile_enable(self._h, 1 if on else 0))

    def pair_kernel_name(self) -> str:
        return self._lib.ljmd_pair_kernel_name(self._h).decode()

    def profile_read(self) -> dict:
        """-> {'pair_ms', 'geometry_ms', 'drift_ms', 'reduce_ms', 'launches'} averages per launch,
        plus '<name>_min': the shortest launch of each interval"""
        ms, lo = (C.c_double * 4)(), (C.c_double * 4)()
        c = C.c_int32()
        self._ck(self._lib.ljmd_profile_read_ex(self._h, ms, lo, C.byref(c)))
        out = {"pair_ms": ms[0], "geometry_ms": ms[1], "drift_ms": ms[2], "reduce_ms": ms[3], "launches": c.value}
        out.update({"pair_ms_min": lo[0], "geometry_ms_min": lo[1], "drift_ms_min": lo[2], "reduce_ms_min": lo[3]})
        return out

    def profile_read_rank(self, rank: int) -> dict:
        """ljmd_profile_read_rank: the same per rank engine, plus the two exchanges of a multi-GPU step
        ('pos_exchange_ms': position all-gather, 'force_exchange_ms': reduce-scatter / all-to-all)"""
        ms, lo, med = (C.c_double * 6)(), (C.c_double * 6)(), (C.c_double * 6)()
        c = C.c_int32()
        self._ck(self._lib.ljmd_profile_read_stats(self._h, rank, ms, lo, med, C.byref(c)))
        names = ("pair_ms", "geometry_ms", "drift_ms", "reduce_ms", "pos_exchange_ms", "force_exchange_ms")
        out = {k: ms[i] for i, k in enumerate(names)}
        out.update({k + "_min": lo[i] for i, k in enumerate(names)})
        out.update({k + "_median": med[i] for i, k in enumerate(names)})
        out["launches"] = c.value
        return out


class BatchEngine:
    """n_replicas independent systems of the same (n, L, dt, rc) on one GPU (ljmd_batch_*, include/ljmd.h): the ensemble
    runs of the reference's run-many framework, one workgroup per replica.  Each replica is the physics of an Engine.
    Per-particle arrays are (B, n) per component, per-replica scalars (B,); n <= 4096.  precision_mode is
    PRECISION_FP64 or PRECISION_FP64_REPRODUCIBLE (per replica the bits of Engine(precision_mode=2) and of
    tests/reproducible_model.py); set_precision changes it later, after which the state has to be set again."""

    BATCH_PRECISION_MODES = (_lib.PRECISION_FP64, _lib.PRECISION_FP64_REPRODUCIBLE)

    def __init__(self, params: SimParams, n_replicas: int, device: int = 0, precision_mode: int = _lib.PRECISION_FP64):
        self._check_mode(precision_mode)
        self._lib = _lib.load()
        self.params = params
        self.n_replicas = int(n_replicas)
        h = C.c_void_p()
        _lib.check_batch(self._lib.ljmd_batch_create(C.byref(h), self.n_replicas, params.n, params.box_length,
                                                     params.dt, params.rc, _lib.PRECISION_FP64, device))
        self._h = h
        self._open_in(precision_mode)

    @classmethod
    def _check_mode(cls, mode) -> None:
        if mode not in cls.BATCH_PRECISION_MODES:
            raise ValueError(f"precision_mode must be one of {cls.BATCH_PRECISION_MODES} for a batch, got {mode!r}")

    def _open_in(self, mode: int) -> None:
        """a new handle is fp64 (the creators take no other mode): switch it, and release it if that fails"""
        self.precision_mode = _lib.PRECISION_FP64
        if mode != _lib.PRECISION_FP64:
            try:
                self.set_precision(mode)
            except Exception:
                self.close()
                raise

    def set_precision(self, mode: int) -> None:
        """ljmd_batch_set_precision: PRECISION_FP64 or PRECISION_FP64_REPRODUCIBLE.  A change of mode drops the resident
        state: set_state has to follow (steps / compute_forces raise LJMD_ERR_STATE until then).  The library, not this
        wrapper, refuses any other mode (LJMD_ERR_INVALID_ARG), and the handle keeps its mode."""
        self._ck(self._lib.ljmd_batch_set_precision(self._h, int(mode)))
        self.precision_mode = int(mode)

    # -- lifecycle ---------------------------------------------------------
    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.ljmd_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _ck(self, status: int) -> None:
        _lib.check_batch(status, self._h)

    def _arrays(self, arrs, name: str):
        shape = (self.n_replicas, self.params.n)
        out = []
        for a in arrs:
            a = np.ascontiguousarray(a, dtype=np.float64)
            if a.shape != shape:
                raise ValueError(f"{name} must have shape {shape}, got {a.shape}")
            out.append(a)
        return out

    # -- state transfer ----------------------------------------------------
    def set_state(self, rx, ry, rz, vx, vy, vz) -> None:
        arrs = self._arrays((rx, ry, rz, vx, vy, vz), "state array")
        self._ck(self._lib.ljmd_batch_set_state(self._h, *[_ptr(a) for a in arrs]))

    def set_accel(self, ax=None, ay=None, az=None) -> None:
        """None = keep that component"""
        ptrs, keep = [], []
        for a in (ax, ay, az):
            if a is None:
                ptrs.append(None)
            else:
                (a,) = self._arrays((a,), "accel array")
                keep.append(a)
                ptrs.append(_ptr(a))
        self._ck(self._lib.ljmd_batch_set_accel(self._h, *ptrs))

    def set_unwrapped(self, ux, uy, uz) -> None:
        arrs = self._arrays((ux, uy, uz), "unwrapped array")
        self._ck(self._lib.ljmd_batch_set_unwrapped(self._h, *[_ptr(a) for a in arrs]))

    def get_state(self, which=("r", "ru", "v", "a")) -> dict:
        """-> {'r': (x, y, z), ...}, each component (B, n)"""
        shape = (self.n_replicas, self.params.n)
        out, ptrs = {}, []
        for key in ("r", "ru", "v", "a"):
            if key in which:
                arrs = tuple(np.empty(shape, dtype=np.float64) for _ in range(3))
                out[key] = arrs
                ptrs += [_ptr(a) for a in arrs]
            else:
                ptrs += [None, None, None]
        self._ck(self._lib.ljmd_batch_get_state(self._h, *ptrs))
        return out

    # -- hot path ----------------------------------------------------------
    def compute_forces(self):
        """-> (epot, d_epot, dd_epot), each (B,)"""
        outs = [np.empty(self.n_replicas, dtype=np.float64) for _ in range(3)]
        self._ck(self._lib.ljmd_batch_compute_forces(self._h, *[_ptr(o) for o in outs]))
        return tuple(outs)

    def kinetic_energy(self) -> np.ndarray:
        out = np.empty(self.n_replicas, dtype=np.float64)
        self._ck(self._lib.ljmd_batch_kinetic_energy(self._h, _ptr(out)))
        return out

    def steps(self, nsteps: int, sample_every: int = 1, observables: bool = True):
        """nsteps Verlet steps of every replica -> (epot, ekin, d_epot, dd_epot), each (nsteps / sample_every, B): the
        scalars of steps sample_every, 2 sample_every, ...; observables=False samples nothing and returns None"""
        if not observables:
            self._ck(self._lib.ljmd_batch_steps(self._h, nsteps, sample_every, None, None, None, None))
            return None
        if sample_every < 1 or nsteps % sample_every != 0:
            raise ValueError("nsteps must be a multiple of sample_every >= 1")
        outs = [np.empty((nsteps // sample_every, self.n_replicas), dtype=np.float64) for _ in range(4)]
        self._ck(self._lib.ljmd_batch_steps(self._h, nsteps, sample_every, *[_ptr(o) for o in outs]))
        return tuple(outs)

    def set_tail_corrections(self, on: bool) -> None:
        self._ck(self._lib.ljmd_batch_set_tail_corrections(self._h, 1 if on else 0))

    def profile_read(self) -> dict:
        """kernel time (ms, HIP events) and launches of the last steps() call"""
        ms, c = C.c_double(), C.c_int32()
        self._ck(self._lib.ljmd_batch_profile_read(self._h, C.byref(ms), C.byref(c)))
        return {"kernel_ms": ms.value, "launches": c.value}

    # -- initial configurations on the device -------------------------------
    def prepare(self, seeds, target_total_energy, warmup_steps: int = 0):
        """ljmd_batch_prepare: every replica gets the reference's initial configuration on the device -- FCC lattice
        (n = 4 k^3), velocities from the reference's generator seeded with -|seed|, centre of mass removed, scaled to
        target_total_energy, warmup_steps Verlet steps, ru <- r -> (epot0, ekin0), each (B,): the energies before the
        scaling.  seeds (integers within int32) and target_total_energy are scalars or B values.  Seeds s, -s and
        3236066 - s give the same velocities.  The handle then has a state and valid accelerations."""
        B = self.n_replicas
        s = np.asarray(seeds)
        if s.dtype == np.bool_ or not np.issubdtype(s.dtype, np.integer):
            raise TypeError(f"prepare: seeds must be integers, got dtype {s.dtype}")
        if s.shape not in ((), (B,)):
            raise ValueError(f"prepare: seeds must be a scalar or have shape ({B},), got {s.shape}")
        if s.size and (int(s.min()) < -2 ** 31 or int(s.max()) > 2 ** 31 - 1):
            raise ValueError("prepare: seeds must lie within the int32 range")
        t = np.asarray(target_total_energy)
        if t.dtype == np.bool_ or not (np.issubdtype(t.dtype, np.floating) or np.issubdtype(t.dtype, np.integer)):
            raise TypeError(f"prepare: target_total_energy must be real numbers, got dtype {t.dtype}")
        if t.shape not in ((), (B,)):
            raise ValueError(f"prepare: target_total_energy must be a scalar or have shape ({B},), got {t.shape}")
        if isinstance(warmup_steps, bool) or not isinstance(warmup_steps, (int, np.integer)):
            raise TypeError(f"prepare: warmup_steps must be an integer, got {warmup_steps!r}")
        if not -2 ** 31 <= int(warmup_steps) <= 2 ** 31 - 1:
            raise ValueError("prepare: warmup_steps must lie within the int32 range")
        s32 = np.ascontiguousarray(np.broadcast_to(s, (B,)), dtype=np.int32)
        t64 = np.ascontiguousarray(np.broadcast_to(t, (B,)), dtype=np.float64)
        epot0 = np.empty(B, dtype=np.float64)
        ekin0 = np.empty(B, dtype=np.float64)
        self._ck(self._lib.ljmd_batch_prepare(self._h, s32.ctypes.data_as(_lib.c_int32_p), _ptr(t64), int(warmup_steps),
                                              _ptr(epot0), _ptr(ekin0)))
        return epot0, ekin0

    # -- g(r) on the device ------------------------------------------------
    def rdf_configure(self, nbins: int, rmax=None, every: int = 0) -> None:
        """ljmd_batch_rdf_configure: nbins bins per replica up to rmax (a scalar, B values, or None = 0.5 L of each
        replica); every > 0: steps() accumulates the positions after steps every, 2 every, ... by itself.  nbins = 0
        switches the feature off.  Zeroes the counts."""
        ptr = None
        if rmax is not None:
            arr = np.ascontiguousarray(np.broadcast_to(np.asarray(rmax, dtype=np.float64), (self.n_replicas,)))
            ptr = _ptr(arr)
        self._ck(self._lib.ljmd_batch_rdf_configure(self._h, int(nbins), ptr, int(every)))
        self._rdf_nbins = int(nbins)

    def rdf_accumulate(self) -> None:
        """adds the pair-distance histogram of every replica's resident positions (no host wait)"""
        self._ck(self._lib.ljmd_batch_rdf_accumulate(self._h))

    def rdf_read(self):
        """-> (hist[B, nbins] uint64, n_snapshots): the counts so far (2 per unordered pair), not cleared"""
        nbins = getattr(self, "_rdf_nbins", 0)
        if nbins < 1:
            raise ValueError("rdf_read: call rdf_configure with nbins >= 1 first")
        hist = np.empty((self.n_replicas, nbins), dtype=np.uint64)
        count = C.c_int64()
        self._ck(self._lib.ljmd_batch_rdf_read(self._h, hist.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(count)))
        return hist, count.value

    def rdf_reset(self) -> None:
        self._ck(self._lib.ljmd_batch_rdf_reset(self._h))

    # -- MSD / VACF on the device ------------------------------------------
    def tcf_configure(self, max_lag: int, origin_stride: int = 1, every: int = 0) -> None:
        """ljmd_batch_tcf_configure: time-origin averaged MSD(tau) and VACF(tau) of every replica up to lag max_lag (in
        snapshots), every origin_stride-th snapshot an origin; every > 0: steps() takes the snapshots after steps every,
        2 every, ... by itself.  max_lag = 0 switches the feature off.  Zeroes the sums."""
        for name, val in (("max_lag", max_lag), ("origin_stride", origin_stride), ("every", every)):
            if isinstance(val, bool) or not isinstance(val, (int, np.integer)):
                raise TypeError(f"tcf_configure: {name} must be an integer, got {val!r}")
        self._ck(self._lib.ljmd_batch_tcf_configure(self._h, int(max_lag), int(origin_stride), int(every)))
        self._tcf_max_lag = int(max_lag)

    def tcf_accumulate(self) -> None:
        """takes every replica's resident ru and v as the next snapshot (no host wait)"""
        self._ck(self._lib.ljmd_batch_tcf_accumulate(self._h))

    def _tcf_rows(self, who: str) -> int:
        max_lag = getattr(self, "_tcf_max_lag", 0)
        if max_lag < 1:
            raise ValueError(f"{who}: call tcf_configure with max_lag >= 1 first")
        return max_lag + 1

    def tcf_read(self):
        """-> (msd[B, max_lag + 1], vacf[B, max_lag + 1], counts[max_lag + 1] int64, n_snapshots); nothing is cleared"""
        rows = self._tcf_rows("tcf_read")
        msd = np.empty((self.n_replicas, rows), dtype=np.float64)
        vacf = np.empty((self.n_replicas, rows), dtype=np.float64)
        counts = np.empty(rows, dtype=np.int64)
        snaps = C.c_int64()
        self._ck(self._lib.ljmd_batch_tcf_read(self._h, _ptr(msd), _ptr(vacf), counts.ctypes.data_as(_lib.c_int64_p),
                                               C.byref(snaps)))
        return msd, vacf, counts, snaps.value

    def tcf_read_exact(self, raw: bool = False):
        """-> (sums, counts, n_snapshots): the exact integer sums of Q(term) = RNE(term 2^64), sums[b, kind, lag] with
        kind 0 = MSD, 1 = VACF, as Python ints in an object array -- or, raw=True, the library's int64 words
        [B, 2, max_lag + 1, 3] (three little-endian limbs of a signed 192-bit integer)"""
        rows = self._tcf_rows("tcf_read_exact")
        words = np.empty((self.n_replicas, 2, rows, 3), dtype=np.int64)
        counts = np.empty(rows, dtype=np.int64)
        snaps = C.c_int64()
        self._ck(self._lib.ljmd_batch_tcf_read_exact(self._h, words.ctypes.data_as(_lib.c_int64_p),
                                                     counts.ctypes.data_as(_lib.c_int64_p), C.byref(snaps)))
        if raw:
            return words, counts, snaps.value
        u = words.view(np.uint64)
        sums = np.empty(words.shape[:3], dtype=object)
        for idx in np.ndindex(*sums.shape):
            sums[idx] = (int(words[idx][2]) << 128) + (int(u[idx][1]) << 64) + int(u[idx][0])
        return sums, counts, snaps.value

    def tcf_reset(self) -> None:
        self._ck(self._lib.ljmd_batch_tcf_reset(self._h))

    # -- pressure tensor on the device (include/ljmd.h: ljmd_batch_stress_*) ----
    def stress_configure(self, max_snapshots: int, every: int = 0) -> None:
        """ljmd_batch_stress_configure: room for max_snapshots snapshots of every replica's pressure tensor on the device;
        every > 0: steps() appends the state after steps every, 2 every, ... by itself.  max_snapshots = 0 switches the
        feature off.  The series starts empty."""
        for name, val in (("max_snapshots", max_snapshots), ("every", every)):
            if isinstance(val, bool) or not isinstance(val, (int, np.integer)):
                raise TypeError(f"stress_configure: {name} must be an integer, got {val!r}")
            if not -2 ** 31 <= int(val) <= 2 ** 31 - 1:
                raise ValueError(f"stress_configure: {name} must lie within the int32 range")
        self._ck(self._lib.ljmd_batch_stress_configure(self._h, int(max_snapshots), int(every)))
        self._stress_max = int(max_snapshots)

    def stress_accumulate(self) -> None:
        """appends the pressure tensor of every replica's resident state to the series (no host wait)"""
        self._ck(self._lib.ljmd_batch_stress_accumulate(self._h))

    def _stress_rows(self, who: str) -> int:
        """snapshots in the series (ljmd_batch_stress_read_exact without a buffer); raises as the reads do"""
        if getattr(self, "_stress_max", 0) < 1:
            raise ValueError(f"{who}: call stress_configure with max_snapshots >= 1 first")
        snaps = C.c_int64()
        self._ck(self._lib.ljmd_batch_stress_read_exact(self._h, None, C.byref(snaps)))
        return snaps.value

    def stress_read(self) -> np.ndarray:
        """-> p[n_snapshots, B, 6]: xx, yy, zz, xy, xz, yz of (sum v v + 12 sum f d) / V_b per snapshot and replica,
        without tail correction; nothing is cleared"""
        p = np.empty((max(self._stress_rows("stress_read"), 1), self.n_replicas, 6), dtype=np.float64)
        snaps = C.c_int64()
        self._ck(self._lib.ljmd_batch_stress_read(self._h, _ptr(p), C.byref(snaps)))
        return p[:snaps.value].copy()

    def stress_read_exact(self, raw: bool = False):
        """-> sums[n_snapshots, B, 12]: the exact integer sums of Q(term) = RNE(term 2^64), K[6] then S[6], as Python
        ints in an object array -- or, raw=True, the library's int64 words [n_snapshots, B, 12, 3] (three little-endian
        limbs of a signed 192-bit integer)"""
        words = np.empty((max(self._stress_rows("stress_read_exact"), 1), self.n_replicas, 12, 3), dtype=np.int64)
        snaps = C.c_int64()
        self._ck(self._lib.ljmd_batch_stress_read_exact(self._h, words.ctypes.data_as(_lib.c_int64_p), C.byref(snaps)))
        words = words[:snaps.value].copy()
        if raw:
            return words
        u = words.view(np.uint64)
        sums = np.empty(words.shape[:3], dtype=object)
        for idx in np.ndindex(*sums.shape):
            sums[idx] = (int(words[idx][2]) << 128) + (int(u[idx][1]) << 64) + int(u[idx][0])
        return sums

    def stress_reset(self) -> None:
        self._ck(self._lib.ljmd_batch_stress_reset(self._h))

    # -- heat flux on the device (include/ljmd.h: ljmd_batch_heatflux_*) --------
    def heatflux_configure(self, max_snapshots: int, every: int = 0) -> None:
        """ljmd_batch_heatflux_configure: room for max_snapshots snapshots of every replica's heat flux on the device;
        every > 0: steps() appends the state after steps every, 2 every, ... by itself.  max_snapshots = 0 switches the
        feature off.  The series starts empty."""
        for name, val in (("max_snapshots", max_snapshots), ("every", every)):
            if isinstance(val, bool) or not isinstance(val, (int, np.integer)):
                raise TypeError(f"heatflux_configure: {name} must be an integer, got {val!r}")
            if not -2 ** 31 <= int(val) <= 2 ** 31 - 1:
                raise ValueError(f"heatflux_configure: {name} must lie within the int32 range")
        self._ck(self._lib.ljmd_batch_heatflux_configure(self._h, int(max_snapshots), int(every)))
        self._heatflux_max = int(max_snapshots)

    def heatflux_accumulate(self) -> None:
        """appends the heat flux of every replica's resident state to the series (no host wait)"""
        self._ck(self._lib.ljmd_batch_heatflux_accumulate(self._h))

    def _heatflux_rows(self, who: str) -> int:
        """snapshots in the series (ljmd_batch_heatflux_read_exact without a buffer); raises as the reads do"""
        if getattr(self, "_heatflux_max", 0) < 1:
            raise ValueError(f"{who}: call heatflux_configure with max_snapshots >= 1 first")
        snaps = C.c_int64()
        self._ck(self._lib.ljmd_batch_heatflux_read_exact(self._h, None, C.byref(snaps)))
        return snaps.value

    def heatflux_read(self):
        """-> (j[n_snapshots, B, 3], parts[n_snapshots, B, 3, 3]): the heat flux (1/2 sum v^2 v + sum phi w +
        6 sum (f . w) d) / V_b per snapshot and replica and its three summands over V_b, parts[..., 0, :] convective,
        parts[..., 1, :] potential, parts[..., 2, :] collisional; nothing is cleared"""
        n = max(self._heatflux_rows("heatflux_read"), 1)
        j = np.empty((n, self.n_replicas, 3), dtype=np.float64)
        parts = np.empty((n, self.n_replicas, 3, 3), dtype=np.float64)
        snaps = C.c_int64()
        self._ck(self._lib.ljmd_batch_heatflux_read(self._h, _ptr(j), _ptr(parts), C.byref(snaps)))
        return j[:snaps.value].copy(), parts[:snaps.value].copy()

    def heatflux_read_exact(self, raw: bool = False):
        """-> sums[n_snapshots, B, 9]: the exact integer sums of Q(term) = RNE(term 2^64), E[3], P[3] then C[3], as
        Python ints in an object array -- or, raw=True, the library's int64 words [n_snapshots, B, 9, 3] (three
        little-endian limbs of a signed 192-bit integer)"""
        words = np.empty((max(self._heatflux_rows("heatflux_read_exact"), 1), self.n_replicas, 9, 3), dtype=np.int64)
        snaps = C.c_int64()
        self._ck(self._lib.ljmd_batch_heatflux_read_exact(self._h, words.ctypes.data_as(_lib.c_int64_p), C.byref(snaps)))
        words = words[:snaps.value].copy()
        if raw:
            return words
        u = words.view(np.uint64)
        sums = np.empty(words.shape[:3], dtype=object)
        for idx in np.ndindex(*sums.shape):
            sums[idx] = (int(words[idx][2]) << 128) + (int(u[idx][1]) << 64) + int(u[idx][0])
        return sums

    def heatflux_reset(self) -> None:
        self._ck(self._lib.ljmd_batch_heatflux_reset(self._h))

    # -- van Hove self-correlation on the device (include/ljmd.h: ljmd_batch_vanhove_*) ----
    def vanhove_configure(self, max_lag: int, origin_stride: int = 1, nbins: int = 128, rmax=None, every: int = 0) -> None:
        """ljmd_batch_vanhove_configure: G_s(r, tau) of every replica up to lag max_lag (in snapshots), every
        origin_stride-th snapshot an origin, nbins bins up to rmax (a scalar, B values, or None = 0.5 L of each replica)
        and an overflow column; every > 0: steps() takes the snapshots after steps every, 2 every, ... by itself.
        max_lag = 0 switches the feature off.  Zeroes everything."""
        for name, val in (("max_lag", max_lag), ("origin_stride", origin_stride), ("nbins", nbins), ("every", every)):
            if isinstance(val, bool) or not isinstance(val, (int, np.integer)):
                raise TypeError(f"vanhove_configure: {name} must be an integer, got {val!r}")
            if not -2 ** 31 <= int(val) <= 2 ** 31 - 1:
                raise ValueError(f"vanhove_configure: {name} must lie within the int32 range")
        B = self.n_replicas
        if rmax is None:
            ps = self.params if isinstance(self.params, (list, tuple)) else [self.params] * B
            arr = np.array([0.5 * p.box_length for p in ps], dtype=np.float64)
        else:
            r = np.asarray(rmax)
            if r.dtype == np.bool_ or not (np.issubdtype(r.dtype, np.floating) or np.issubdtype(r.dtype, np.integer)):
                raise TypeError(f"vanhove_configure: rmax must be real numbers, got dtype {r.dtype}")
            if r.shape not in ((), (B,)):
                raise ValueError(f"vanhove_configure: rmax must be a scalar or have shape ({B},), got {r.shape}")
            arr = np.ascontiguousarray(np.broadcast_to(r, (B,)), dtype=np.float64)
        self._ck(self._lib.ljmd_batch_vanhove_configure(self._h, int(max_lag), int(origin_stride), int(nbins), _ptr(arr),
                                                        int(every)))
        self._vanhove_shape = (int(max_lag), int(nbins))

    def vanhove_accumulate(self) -> None:
        """takes every replica's resident ru as the next snapshot (no host wait)"""
        self._ck(self._lib.ljmd_batch_vanhove_accumulate(self._h))

    def _vanhove_rows(self, who: str):
        max_lag, nbins = getattr(self, "_vanhove_shape", (0, 0))
        if max_lag < 1:
            raise ValueError(f"{who}: call vanhove_configure with max_lag >= 1 first")
        return max_lag + 1, nbins + 1

    def _vanhove_ck(self, status: int, result):
        """as _ck; a range error (LJMD_ERR_RANGE) carries the arrays, which the library has filled, in its `result`"""
        try:
            self._ck(status)
        except _lib.LjmdError as e:
            if e.code == _lib.LJMD_ERR_RANGE:
                e.result = result()
            raise
        return result()

    def vanhove_read(self):
        """-> (hist[B, max_lag + 1, nbins + 1] uint64 with the overflow column last, r2[B, max_lag + 1],
        r4[B, max_lag + 1], counts[max_lag + 1] int64, n_snapshots); nothing is cleared"""
        rows, cols = self._vanhove_rows("vanhove_read")
        B = self.n_replicas
        hist = np.empty((B, rows, cols), dtype=np.uint64)
        r2 = np.empty((B, rows), dtype=np.float64)
        r4 = np.empty((B, rows), dtype=np.float64)
        counts = np.empty(rows, dtype=np.int64)
        snaps = C.c_int64()
        st = self._lib.ljmd_batch_vanhove_read(self._h, hist.ctypes.data_as(C.POINTER(C.c_uint64)), _ptr(r2), _ptr(r4),
                                               counts.ctypes.data_as(_lib.c_int64_p), C.byref(snaps))
        return self._vanhove_ck(st, lambda: (hist, r2, r4, counts, snaps.value))

    def vanhove_read_exact(self, raw: bool = False):
        """-> (hist, sums, counts, n_snapshots): the counts and the exact integer sums of Q(t) = RNE(t 2^64),
        sums[b, kind, lag] with kind 0 = r^2, 1 = r^4, as Python ints in an object array -- or, raw=True, the library's
        int64 words [B, 2, max_lag + 1, 3] (three little-endian limbs of a signed 192-bit integer)"""
        rows, cols = self._vanhove_rows("vanhove_read_exact")
        B = self.n_replicas
        hist = np.empty((B, rows, cols), dtype=np.uint64)
        words = np.empty((B, 2, rows, 3), dtype=np.int64)
        counts = np.empty(rows, dtype=np.int64)
        snaps = C.c_int64()
        st = self._lib.ljmd_batch_vanhove_read_exact(self._h, hist.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                     words.ctypes.data_as(_lib.c_int64_p),
                                                     counts.ctypes.data_as(_lib.c_int64_p), C.byref(snaps))

        def result():
            if raw:
                return hist, words, counts, snaps.value
            u = words.view(np.uint64)
            sums = np.empty(words.shape[:3], dtype=object)
            for idx in np.ndindex(*sums.shape):
                sums[idx] = (int(words[idx][2]) << 128) + (int(u[idx][1]) << 64) + int(u[idx][0])
            return hist, sums, counts, snaps.value
        return self._vanhove_ck(st, result)

    def vanhove_reset(self) -> None:
        self._ck(self._lib.ljmd_batch_vanhove_reset(self._h))

    # -- density modes on the device (include/ljmd.h: ljmd_batch_rhok_*) ---------
    def rhok_configure(self, modes, max_snapshots: int, every: int = 0) -> None:
        """ljmd_batch_rhok_configure: one mode list for the handle (integer triples [n_modes, 3], k_b = 2 pi n / L_b;
        Engine.rhok_select_modes gives the drivers' list) and room for max_snapshots snapshots of every replica's rho_k
        on the device; every > 0: steps() appends the state after steps every, 2 every, ... by itself.  max_snapshots = 0
        switches the feature off.  The series starts empty."""
        for name, val in (("max_snapshots", max_snapshots), ("every", every)):
            if isinstance(val, bool) or not isinstance(val, (int, np.integer)):
                raise TypeError(f"rhok_configure: {name} must be an integer, got {val!r}")
            if not -2 ** 31 <= int(val) <= 2 ** 31 - 1:
                raise ValueError(f"rhok_configure: {name} must lie within the int32 range")
        m = np.asarray(modes if modes is not None else np.zeros((0, 3)))
        if m.size and not np.issubdtype(m.dtype, np.integer):
            raise TypeError("rhok_configure: modes must be integers")
        if m.ndim != 2 or m.shape[1] != 3:
            raise ValueError(f"rhok_configure: modes must have shape [n_modes, 3], got {m.shape}")
        if m.size and np.abs(m).max() > np.iinfo(np.int32).max:
            raise ValueError("rhok_configure: modes must lie within the int32 range")
        m = np.ascontiguousarray(m, dtype=np.int32)
        self._ck(self._lib.ljmd_batch_rhok_configure(self._h, m.shape[0], m.ctypes.data_as(_lib.c_int32_p) if m.size else None,
                                                     int(max_snapshots), int(every)))
        self._rhok_modes = m.shape[0] if int(max_snapshots) > 0 else 0

    def rhok_accumulate(self) -> None:
        """appends rho_k of every replica's resident positions to the series (no host wait)"""
        self._ck(self._lib.ljmd_batch_rhok_accumulate(self._h))

    def _rhok_count(self) -> int:
        """snapshots in the series (ljmd_batch_rhok_read_exact without a buffer); raises as the reads do"""
        snaps = C.c_int64()
        self._ck(self._lib.ljmd_batch_rhok_read_exact(self._h, None, C.byref(snaps)))
        return snaps.value

    def rhok_read(self) -> np.ndarray:
        """-> rho[n_snapshots, B, n_modes] complex: sum_j (cos k.r_j + i sin k.r_j) per replica, each part one rounding
        of its exact integer; nothing is cleared"""
        n, m = max(self._rhok_count(), 1), max(getattr(self, "_rhok_modes", 0), 1)
        rho = np.empty((n, self.n_replicas, m, 2), dtype=np.float64)
        snaps = C.c_int64()
        self._ck(self._lib.ljmd_batch_rhok_read(self._h, _ptr(rho), C.byref(snaps)))
        return rho[:snaps.value].copy().view(np.complex128)[..., 0]

    def rhok_read_exact(self, raw: bool = False):
        """-> sums[n_snapshots, B, n_modes, 2]: the exact integer sums of Q(cos) and Q(sin), Q(t) = RNE(t 2^64), as
        Python ints in an object array -- or, raw=True, the library's int64 words [n_snapshots, B, n_modes, 2, 3] (three
        little-endian limbs of a signed 192-bit integer)"""
        m = max(getattr(self, "_rhok_modes", 0), 1)
        words = np.empty((max(self._rhok_count(), 1), self.n_replicas, m, 2, 3), dtype=np.int64)
        snaps = C.c_int64()
        self._ck(self._lib.ljmd_batch_rhok_read_exact(self._h, words.ctypes.data_as(_lib.c_int64_p), C.byref(snaps)))
        words = words[:snaps.value].copy()
        if raw:
            return words
        u = words.view(np.uint64)
        sums = np.empty(words.shape[:4], dtype=object)
        for idx in np.ndindex(*sums.shape):
            sums[idx] = (int(words[idx][2]) << 128) + (int(u[idx][1]) << 64) + int(u[idx][0])
        return sums

    def rhok_reset(self) -> None:
        self._ck(self._lib.ljmd_batch_rhok_reset(self._h))

    def rhok_profile(self) -> dict:
        """ljmd_batch_rhok_profile_read for the most recent rhok_accumulate -> {'kernel_ms'}"""
        ms = C.c_double()
        self._ck(self._lib.ljmd_batch_rhok_profile_read(self._h, C.byref(ms)))
        return {"kernel_ms": ms.value}

    @staticmethod
    def per_replica(params_list, device: int = 0,
                    precision_mode: int = _lib.PRECISION_FP64) -> "PerReplicaBatchEngine":
        """one handle of len(params_list) replicas, replica b with its own (n, L, dt, rc) = params_list[b]"""
        return PerReplicaBatchEngine(params_list, device, precision_mode)


class PerReplicaBatchEngine(BatchEngine):
    """BatchEngine whose replicas each have their own SimParams (ljmd_batch_create_per_replica): a sweep over state
    points or sizes in one handle.  Replica b's results equal those of a one-replica BatchEngine of params_list[b].
    Per-particle arguments and results are lists of B arrays of shape (n_b,); per-replica scalars stay (B,) and the
    scalars of steps() (samples, B).  offsets[b] .. offsets[b + 1] is replica b's range in the library's planes."""

    def __init__(self, params_list, device: int = 0, precision_mode: int = _lib.PRECISION_FP64):
        self._check_mode(precision_mode)
        self._lib = _lib.load()
        self.params_list = list(params_list)
        self.n_replicas = len(self.params_list)
        if self.n_replicas < 1:
            raise ValueError("params_list must hold at least one SimParams")
        n = np.array([p.n for p in self.params_list], dtype=np.int32)
        box = np.array([p.box_length for p in self.params_list], dtype=np.float64)
        dt = np.array([p.dt for p in self.params_list], dtype=np.float64)
        rc = np.array([p.rc for p in self.params_list], dtype=np.float64)
        h = C.c_void_p()
        _lib.check_batch(self._lib.ljmd_batch_create_per_replica(
            C.byref(h), self.n_replicas, n.ctypes.data_as(_lib.c_int32_p), _ptr(box), _ptr(dt), _ptr(rc),
            _lib.PRECISION_FP64, device))
        self._h = h
        off = np.empty(self.n_replicas + 1, dtype=np.int64)
        self._ck(self._lib.ljmd_batch_offsets(self._h, off.ctypes.data_as(_lib.c_int64_p)))
        self.offsets = off
        self._open_in(precision_mode)

    @property
    def params(self):
        return self.params_list

    def _arrays(self, arrs, name: str):
        """each of arrs: B arrays, replica b's of shape (n_b,) -> one concatenated array per component"""
        out = []
        for a in arrs:
            if isinstance(a, np.ndarray) or len(a) != self.n_replicas:
                raise ValueError(f"{name} must be a list of {self.n_replicas} arrays (one per replica)")
            parts = []
            for b, x in enumerate(a):
                x = np.ascontiguousarray(x, dtype=np.float64)
                nb = int(self.offsets[b + 1] - self.offsets[b])
                if x.shape != (nb,):
                    raise ValueError(f"{name} of replica {b} must have shape ({nb},), got {x.shape}")
                parts.append(x)
            out.append(np.concatenate(parts))
        return out

    def _split(self, flat: np.ndarray):
        return [flat[self.offsets[b]:self.offsets[b + 1]] for b in range(self.n_replicas)]

    def get_state(self, which=("r", "ru", "v", "a")) -> dict:
        """-> {'r': (x, y, z), ...}, each component a list of B arrays (n_b,)"""
        total = int(self.offsets[-1])
        out, ptrs = {}, []
        for key in ("r", "ru", "v", "a"):
            if key in which:
                arrs = tuple(np.empty(total, dtype=np.float64) for _ in range(3))
                out[key] = tuple(self._split(a) for a in arrs)
                ptrs += [_ptr(a) for a in arrs]
            else:
                ptrs += [None, None, None]
        self._ck(self._lib.ljmd_batch_get_state(self._h, *ptrs))
        return out


def observables(params: SimParams, epot: float, ekin: float, d_epot: float):
    """etot, T, P of one sample: md_simulation_program.f90:355,366 + md_means.f90:215-228.
    Note T uses 3N (not 3N-3) in the time series."""
    npd = float(params.n)
    rho = npd / params.volume
    virial = -d_epot
    etot = epot + ekin
    temp = 2.0 * ekin / (3.0 * npd)
    press = rho * temp + virial / (3.0 * params.volume)
    return etot, temp, press
