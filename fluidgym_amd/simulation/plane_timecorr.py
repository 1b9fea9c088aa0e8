"""Online temporal two-point correlations of wall-parallel planes: how long a wall distance remembers itself.

The reference records these with ``TemporalTwoPointCorrelation_Online_torch`` (``pict/data/online_statistics.py:1271-1343``), fed by
``TCF_tools.VelocityStats.record_vel_stats`` (``:1508-1511``), plotted as ``R(ETT) / R(0)`` (``:1090-1194``) and saved as
``online_stats_vel_temporal.npz`` (``:1781-1784``): the fluctuation ``c' = c - mean_{z,x}(c)`` of the first sample is cloned as the
base ``b'``, and every sample appends ``mean(b' c') / (rms(b') rms(c'))`` per (env, component, row ``y``).  One base of one
realisation; its own averaging over windows is switched off (``average_stats = False  # gives wrong results``, ``:1102``).

Here one sample of a batch of ``B`` envs is one launch of ``fg_plane_timecorr`` (``csrc/fg_planetimecorr.hip``) that leaves nothing on
the host, and a record can keep several staggered bases: with ``stride = S`` a new base starts at every ``S``-th sample in slot
``(s // S) % n_slots`` of a ring of ``n_slots = ceil(lags / S) <= 8`` slots and contributes the lag ``s - s0`` while that is below
``lags``; ``stride = None`` is the reference's single base at the first sample (after ``lags`` samples the record is ``full`` and
further samples are dropped).  Every env is its own realisation; ``pooled()`` sums them.

A record holds ``acc [B, ny, K, lags, 4]`` -- per lag the sums over the contributing bases of the coefficient, of ``mean(b' c')``,
of ``mean(b'^2)`` and of ``mean(c'^2)`` -- and on the host, because the schedule is deterministic, ``count [lags]`` (bases behind a
lag), ``time_sum [B, lags]`` (their elapsed times) and the sample times.  Sums make a merge an addition.  A stored base is rounded
to the dtype of the fields, and its own ``sum b'^2`` and lag-0 cross term are taken from the rounded values.

Memory: one slot is ``B * K * nz * ny * nx * itemsize`` bytes -- ``8 * 3 * 64 * 64 * 128 * 4`` = 50 MB for ``TCF3D-baseline`` x 8 envs
with the three velocity components in fp32 -- and a record holds ``n_slots`` of them.

``PlaneTimeCorrelation`` accumulates on the GPU, ``HostPlaneTimeCorrelation`` is its NumPy fp64 twin (the reference of the tests);
both share the accessors, ``merge`` / ``pooled``, the wall units and ``save``.
"""
from __future__ import annotations

import ctypes
import json
import os
from typing import List, Optional, Sequence, Union

import numpy as np
import torch

from .. import _lib as L
from . import plane_fields as F
from .plane_fields import gather as _gather
from .plane_spectra import CHANNEL_NAMES
from .plane_stats import PlaneRecord

MAX_SLOTS = 8
FILE_RECORD, FILE_META, FILE_REFERENCE = "plane_timecorr.npz", "plane_timecorr.json", "online_stats_vel_temporal.npz"


def sample_timecorr(values: np.ndarray, slot_lag: Sequence[int], base: np.ndarray, base_ss: np.ndarray, acc: np.ndarray) -> None:
    """One sample on the host, in place, as ``fg_plane_timecorr`` takes it: ``values [B, K, nz, ny, nx]``,
    ``base [n_slots, B, K, nz, ny, nx]`` (its dtype is the rounding of a stored base), ``base_ss [n_slots, B, ny, K]``,
    ``acc [B, ny, K, lags, 4]``."""
    v = np.asarray(values, np.float64)
    cells = v.shape[2] * v.shape[4]
    with np.errstate(all="ignore"):
        c = v - (v.sum(axis=(2, 4)) / cells)[:, :, None, :, None]
        cc = np.moveaxis((c * c).sum(axis=(2, 4)), 1, 2)                          # [B, ny, K]
        for j, lag in enumerate(slot_lag):
            if lag < 0:
                continue
            if lag == 0:
                base[j] = c.astype(base.dtype)
                b = base[j].astype(np.float64)
                base_ss[j] = np.moveaxis((b * b).sum(axis=(2, 4)), 1, 2)
            else:
                b = base[j].astype(np.float64)
            cross = np.moveaxis((b * c).sum(axis=(2, 4)), 1, 2)
            lost = ~(np.isfinite(cross) & np.isfinite(base_ss[j]) & np.isfinite(cc))      # a non-finite cell in the sample or the base
            for q, add in enumerate((cross / np.sqrt(base_ss[j] * cc), cross / cells, base_ss[j] / cells, cc / cells)):
                acc[..., lag, q] += np.where(lost, np.nan, add)


class TimeCorrRecord:
    """Schedule, accessors, merging, wall units and files of a record; the two accumulators below say where the arrays live."""

    def __init__(self, channels: Sequence[str] = ("u", "v", "w"), lags: int = 1, stride: Optional[int] = None):
        channels = tuple(channels)
        if not channels or len(set(channels)) != len(channels) or any(c not in CHANNEL_NAMES for c in channels):
            raise ValueError(f"channels must be distinct names out of {CHANNEL_NAMES}, got {channels}")
        if int(lags) < 1:
            raise ValueError(f"lags must be at least 1, got {lags}")
        if stride is not None and int(stride) < 1:
            raise ValueError(f"stride must be None (one base at the first sample) or at least 1, got {stride}")
        self.channels, self.lags = channels, int(lags)
        self.stride = None if stride is None else int(stride)
        self.K = len(channels)
        self.n_slots = 1 if stride is None else -(-self.lags // self.stride)
        if self.n_slots > MAX_SLOTS:
            raise ValueError(f"lags = {lags} with stride = {stride} needs {self.n_slots} base slots, more than the {MAX_SLOTS} that "
                             f"fg_plane_timecorr takes: raise the stride to at least {-(-self.lags // MAX_SLOTS)}")
        self.samples = 0                                   # samples seen (the dropped ones of a full single-base record included)
        self.count = np.zeros(self.lags)                   # bases that have contributed to a lag (the same for every env)
        self.time_sum: Optional[np.ndarray] = None         # [B, lags]: their elapsed times
        self.times: List[np.ndarray] = []                  # [B] per recorded sample
        self._slot_time: Optional[np.ndarray] = None       # [n_slots, B]: when the base of a slot was taken
        self._slot_start = [-1] * self.n_slots             # the sample at which it was taken
        self.grid: Optional[tuple] = None                  # (nz, ny, nx) once known
        self.y_centers: Optional[np.ndarray] = None        # wall units, as PlaneRecord
        self.viscosity: Optional[float] = None
        self._u_wall: Optional[np.ndarray] = None

    # ---- the schedule
    @property
    def full(self) -> bool:
        """A single-base record that has seen all its lags: further samples are dropped."""
        return self.stride is None and self.samples >= self.lags

    def slot_lags(self, s: int) -> List[int]:
        """What every slot does at sample ``s`` (the ``slot_lag`` table of ``fg_plane_timecorr``), before the sample is counted."""
        out = []
        for j in range(self.n_slots):
            if self.stride is None:
                start = 0 if j == 0 else -1
            else:
                start = s if (s % self.stride == 0 and (s // self.stride) % self.n_slots == j) else self._slot_start[j]
            out.append(s - start if 0 <= start <= s and s - start < self.lags else -1)
        return out

    def _advance(self, time, B: int) -> Optional[List[int]]:
        """Book one sample at ``time`` (a scalar or ``[B]``); the slot table to record it with, or None when it is dropped."""
        t = np.broadcast_to(np.asarray(time, np.float64), (B,)).copy()
        if self.time_sum is None:
            self.time_sum, self._slot_time = np.zeros((B, self.lags)), np.zeros((self.n_slots, B))
        s = self.samples
        self.samples += 1
        table = self.slot_lags(s)
        if all(lag < 0 for lag in table):
            return None
        self.times.append(t)
        for j, lag in enumerate(table):
            if lag == 0:
                self._slot_start[j], self._slot_time[j] = s, t
            if lag >= 0:
                self.count[lag] += 1.0
                self.time_sum[:, lag] += t - self._slot_time[j]
        return table

    def _take_grid(self, B: int, nz: int, ny: int, nx: int, what: str) -> None:
        if self.grid is None:
            self.grid = (nz, ny, nx)
        elif self.grid != (nz, ny, nx) or self.time_sum.shape[0] != B:
            raise ValueError(f"{what}: batch size or grid changed between updates")

    # ---- where the arrays live: overridden by PlaneTimeCorrelation
    _acc = _base = _base_ss = None

    def _state(self) -> np.ndarray:
        if self._acc is None:
            raise RuntimeError("no sample recorded yet")
        return self._acc

    def _set_state(self, acc) -> None:
        self._acc = np.ascontiguousarray(acc, np.float64)

    def _bases(self):
        """(base [n_slots, B, K, nz, ny, nx], base_ss [n_slots, B, ny, K]) on the host."""
        self._state()
        return self._base, self._base_ss

    def _unset(self) -> bool:
        return self._acc is None

    def _like(self, acc, count, time_sum) -> "HostPlaneTimeCorrelation":
        r = HostPlaneTimeCorrelation(self.channels, self.lags, self.stride)
        r._set_state(acc)
        r.count, r.time_sum = np.array(count, np.float64), np.array(time_sum, np.float64)
        r.samples, r.times, r.grid = self.samples, list(self.times), self.grid
        r.y_centers, r.viscosity, r._u_wall = self.y_centers, self.viscosity, self._u_wall
        return r

    def record(self) -> "HostPlaneTimeCorrelation":
        """A host copy of the sums (not of the bases: it serves the accessors, ``merge`` and ``pooled``)."""
        return self._like(np.array(self._state()), self.count, self.time_sum)

    # ---- accessors: [B, ny, lags] each
    def _ch(self, ch: Union[int, str]) -> int:
        return self.channels.index(ch) if isinstance(ch, str) else int(ch)

    def _sum(self, ch, q: int) -> np.ndarray:
        return self._state()[:, :, self._ch(ch), :, q]

    def coefficient(self, ch) -> np.ndarray:
        """The reference's coefficient ``mean(b' c') / (rms(b') rms(c'))``, averaged over the bases that reached a lag."""
        with np.errstate(all="ignore"):
            return self._sum(ch, 0) / self.count

    def correlation(self, ch) -> np.ndarray:
        """The ratio of the pooled sums, ``sum cross / sqrt(sum var_base sum var_cur)``: the better estimator with several bases."""
        with np.errstate(all="ignore"):
            return self._sum(ch, 1) / np.sqrt(self._sum(ch, 2) * self._sum(ch, 3))

    def normalized(self, ch) -> np.ndarray:
        """``R(lag) / R(0)`` of the coefficient: what the reference plots."""
        c = self.coefficient(ch)
        with np.errstate(all="ignore"):
            return c / c[..., :1]

    def lag_time(self) -> np.ndarray:
        """Mean elapsed time between a base and its sample per lag, ``[B, lags]``."""
        if self.time_sum is None:
            raise RuntimeError("no sample recorded yet")
        with np.errstate(all="ignore"):
            return self.time_sum / self.count

    def integral_time(self, ch) -> np.ndarray:
        """Trapezoid of ``correlation`` over ``lag_time`` up to the first zero crossing (the last interval ends where the straight
        line between its two lags crosses zero), or up to the last recorded lag when there is none; ``[B, ny]``."""
        r, t = self.correlation(ch), self.lag_time()
        n = int(np.count_nonzero(self.count))
        out = np.full(r.shape[:2], np.nan)
        for b, y in np.ndindex(*out.shape):
            total = 0.0
            for i in range(1, n):
                r0, r1, dt = r[b, y, i - 1], r[b, y, i], t[b, i] - t[b, i - 1]
                if not r1 > 0.0:                           # the crossing (or a NaN, which ends the integral as NaN)
                    total += 0.5 * r0 * dt * (r0 / (r0 - r1))
                    break
                total += 0.5 * (r0 + r1) * dt
            out[b, y] = total
        return out

    # ---- wall units: y+ by PlaneRecord's helper; a correlation has no mean profile, so the friction velocity is given
    def set_wall_units(self, y_centers, viscosity: float, u_wall) -> "TimeCorrRecord":
        PlaneRecord.set_wall_units(self, y_centers, viscosity)
        self._u_wall = np.atleast_1d(np.asarray(u_wall, np.float64)).copy()
        return self

    _need_wall = PlaneRecord._need_wall
    to_wall_pos = PlaneRecord.to_wall_pos

    def u_wall(self) -> np.ndarray:
        self._need_wall()
        return self._u_wall

    def lag_ETT(self) -> np.ndarray:
        """``lag_time`` in eddy turnover times ``t u_wall / delta`` (``t_to_ETT``, TCF_tools.py:45-46; half width ``delta = 1``)."""
        return self.lag_time() * self.u_wall()[:, None]

    def lag_t_wall(self) -> np.ndarray:
        """``lag_time`` in viscous units, ``t+ = t u_wall^2 / nu`` (``t_to_t_wall``, TCF_tools.py:54-59)."""
        return self.lag_time() * (self.u_wall() ** 2 / self._need_wall()[1])[:, None]

    # ---- merging
    def merge(self, other: "TimeCorrRecord") -> "TimeCorrRecord":
        """Add ``other``'s sums (same channels, lags, stride, batch size and grid) to this record, env by env."""
        if (other.channels, other.lags, other.stride) != (self.channels, self.lags, self.stride):
            raise ValueError("merge: both records need the same channels, lags and stride")
        aB = other._state()
        if self._unset():
            raise RuntimeError("merge: this record has no sample yet (merge into other.record() instead)")
        aA = self._state()
        if aA.shape != aB.shape or self.grid != other.grid:
            raise ValueError(f"merge: shapes differ, {aA.shape} and {aB.shape}")
        self._set_state(aA + aB)
        self.count = self.count + other.count
        self.time_sum = self.time_sum + other.time_sum
        return self

    def pooled(self) -> "HostPlaneTimeCorrelation":
        """The envs of the batch summed into one ensemble record (``B = 1``) on the host: ``B`` times the bases per lag."""
        acc = self._state()
        B = acc.shape[0]
        r = self._like(acc.sum(axis=0, keepdims=True), self.count * B, self.time_sum.sum(axis=0, keepdims=True))
        if r._u_wall is not None and len(r._u_wall) == B:
            r._u_wall = r._u_wall.mean(keepdims=True)
        return r

    # ---- files
    def reference_arrays(self) -> dict:
        """What ``TemporalTwoPointCorrelation_Online_torch.save`` writes, with the batch kept: ``base_fluctuations [B, C, Z, Y, X]``,
        ``base_rms [B, C, ny]``, ``steps_coefficients [steps, B, C, ny]``, ``steps_time [steps]`` of env 0, and the times of every env
        as ``steps_time_envs [steps, B]``.  A single-base record of the velocity components only."""
        if self.stride is not None or any(c not in "uvw" for c in self.channels):
            raise ValueError("the reference's file is that of one base of the velocity: stride None, channels out of u, v, w")
        base, base_ss = self._bases()
        nz, _, nx = self.grid
        steps = len(self.times)
        times = np.stack(self.times)
        return {"base_fluctuations": np.array(base[0]), "base_rms": np.sqrt(np.moveaxis(base_ss[0], 1, 2) / (nz * nx)),
                "steps_coefficients": np.moveaxis(self._state()[..., :steps, 0], (3, 2), (0, 2)).copy(),
                "steps_time": times[:, 0].copy(), "steps_time_envs": times}

    def save(self, directory) -> None:
        """``plane_timecorr.npz`` (the sums, the counts, the times) and ``plane_timecorr.json`` (channels, schedule, wall units) into
        ``directory``; a single-base record of velocity components also writes the reference's ``online_stats_vel_temporal.npz``."""
        os.makedirs(str(directory), exist_ok=True)
        acc = self._state()
        times = np.stack(self.times) if self.times else np.zeros((0, acc.shape[0]))
        np.savez_compressed(os.path.join(str(directory), FILE_RECORD), acc=acc, count=self.count, time_sum=self.time_sum, times=times)
        reference = self.stride is None and all(c in "uvw" for c in self.channels)
        meta = {"channels": list(self.channels), "lags": self.lags, "stride": self.stride, "n_slots": self.n_slots,
                "samples": self.samples, "grid": None if self.grid is None else list(self.grid), "reference_file": reference,
                "y_centers": None if self.y_centers is None else [float(v) for v in self.y_centers], "viscosity": self.viscosity,
                "u_wall": None if self._u_wall is None else [float(v) for v in self._u_wall]}
        with open(os.path.join(str(directory), FILE_META), "w") as f:
            json.dump(meta, f, indent=1)
        if reference:
            np.savez_compressed(os.path.join(str(directory), FILE_REFERENCE), **self.reference_arrays())

    @staticmethod
    def load(directory) -> "HostPlaneTimeCorrelation":
        """The sums ``save`` wrote (not the bases: the loaded record serves the accessors, ``merge`` and ``pooled``)."""
        with open(os.path.join(str(directory), FILE_META)) as f:
            meta = json.load(f)
        r = HostPlaneTimeCorrelation(tuple(meta["channels"]), meta["lags"], meta["stride"])
        with np.load(os.path.join(str(directory), FILE_RECORD)) as z:
            r._set_state(z["acc"])
            r.count, r.time_sum, r.times = z["count"], z["time_sum"], list(z["times"])
        r.samples, r.grid = int(meta["samples"]), None if meta["grid"] is None else tuple(meta["grid"])
        if meta.get("y_centers") is not None:
            r.set_wall_units(meta["y_centers"], meta["viscosity"], meta["u_wall"])
        return r


class HostPlaneTimeCorrelation(TimeCorrRecord):
    """The NumPy fp64 twin of ``PlaneTimeCorrelation``: same schedule and arithmetic, arrays on the host; a stored base is rounded
    to the dtype of the fields it was taken from, as on the device."""

    def update(self, velocity, pressure=None, scalar=None, time=0.0) -> None:
        what = "HostPlaneTimeCorrelation.update"
        velocity = np.asarray(velocity)
        pressure, scalar = (None if t is None else np.asarray(t) for t in (pressure, scalar))
        fields = [t[:, c] for t, c in _gather(self.channels, velocity, pressure, scalar, what)]
        v = np.stack(fields, axis=1)                                              # [B, K, (Z,) Y, X]
        if v.ndim == 4:
            v = v[:, :, None]
        B, _, nz, ny, nx = v.shape
        if self.grid is not None:
            self._take_grid(B, nz, ny, nx, what)
        table = self._advance(time, B)
        self._take_grid(B, nz, ny, nx, what)
        if self._acc is None:
            dtype = velocity.dtype if velocity.dtype in (np.float32, np.float64) else np.float64
            self._acc = np.zeros((B, ny, self.K, self.lags, 4))
            self._base = np.zeros((self.n_slots,) + v.shape, dtype)
            self._base_ss = np.zeros((self.n_slots, B, ny, self.K))
        if table is not None:
            sample_timecorr(v, table, self._base, self._base_ss, self._acc)


class PlaneTimeCorrelation(F.DeviceState, TimeCorrRecord):
    """The GPU accumulator.  ``update(velocity, pressure=None, scalar=None, time=...)`` takes the domain's own tensors
    (``[B, d, (Z,) Y, X]``, ``[B, 1, ...]``, ``[B, S, ...]``; float32 -> ``libfluidgym_hip.so``, float64 -> the fp64 library), reads
    their component slices in place and runs one launch on the current stream; ``time`` is a host scalar or per-env array, and nothing
    comes back to the host until an accessor is called."""

    _merge_into = "a record()"
    # _dev: (acc [B, ny, K, lags, 4], base [n_slots, B, K, nz, ny, nx], base_ss [n_slots, B, ny, K]) on the device

    def _state(self) -> np.ndarray:
        return self._read(1)[0]

    def _set_state(self, acc) -> None:
        self._write(acc)

    def _bases(self):
        self._state()
        return self._dev[1].cpu().numpy(), self._dev[2].cpu().numpy()

    def update(self, velocity: torch.Tensor, pressure: Optional[torch.Tensor] = None, scalar: Optional[torch.Tensor] = None,
               time=0.0) -> None:
        what = "PlaneTimeCorrelation.update"
        used = (velocity,) + ((pressure,) if "p" in self.channels else ()) + ((scalar,) if "T" in self.channels else ())
        F.check_device_fields(used, what, "HostPlaneTimeCorrelation")
        parts = [(t.contiguous(), c) for t, c in _gather(self.channels, velocity, pressure, scalar, what)]
        B, nz, ny, nx = F.grid_of(velocity)
        dev = velocity.device
        if self._dev is not None and self._shape != (B, nz, ny, nx, dev, velocity.dtype):
            raise ValueError(f"{what}: batch size, grid, dtype or device changed between updates")
        table = self._advance(time, B)
        if self._dev is None:
            self._take_grid(B, nz, ny, nx, what)
            self._shape = (B, nz, ny, nx, dev, velocity.dtype)
            self._dev = (torch.zeros(B, ny, self.K, self.lags, 4, dtype=torch.float64, device=dev),
                         torch.zeros(self.n_slots, B, self.K, nz, ny, nx, dtype=velocity.dtype, device=dev),
                         torch.zeros(self.n_slots, B, ny, self.K, dtype=torch.float64, device=dev))
        if table is None:
            return
        ptrs, strides = F.channel_table(parts, nz * ny * nx)
        slots = (ctypes.c_int32 * self.n_slots)(*table)
        lib = F.library(velocity.dtype)
        acc, base, base_ss = self._dev
        with torch.cuda.device(dev):
            L.check(lib.fg_plane_timecorr(ptrs, strides, self.K, B, nz, ny, nx, self.lags, self.n_slots, slots, F.ptr(base), F.ptr(base_ss),
                                          F.ptr(acc), F.stream_ptr(dev)), lib=lib)
