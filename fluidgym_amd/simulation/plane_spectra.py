"""Online wavenumber spectra of wall-parallel planes: at which scales the fluctuations of a wall distance live.

The reference accumulates these with ``PSDOnline_Torch`` (``pict/data/online_statistics.py:269-416``), fed by
``TCF_tools.VelocityStats.record_vel_stats`` when ``PSD_planes`` are given (``:445-459, 1491-1500``): ``|fftn(velocity)|`` over z and
x on the chosen rows ``y`` and their mirror images, cut to the lower half of the wavenumbers, averaged over the batch and kept as a
running mean over the samples.  Here one sample of a batch of ``B`` envs is one launch of ``fg_plane_spectra``
(``csrc/fg_planespectra.hip``) that adds ``|u^|`` and ``|u^|^2`` of every (env, channel, plane) into fp64 running sums on the GPU.

A record holds the sums ``amp`` and ``power`` ``[B, K, T, nkz, nkx]`` (``T`` table entries: the planes, then their mirrors when
``symmetric``; ``nkz = max(nz / 2, 1)``, ``nkx = nx / 2``) and ``count [B]``, the env-samples behind every batch entry; sums make a
merge an addition.  ``PlaneSpectra`` accumulates on the GPU, ``HostPlaneSpectra`` is its NumPy fp64 twin; both share the accessors,
``merge`` / ``pooled``, the pre-multiplied spectra of ``PSDOnline_Torch.get_phi`` and ``save`` in the reference's file layout.
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
from .plane_fields import gather as _gather      # (the correlations take it from here)

CHANNEL_NAMES = ("u", "v", "w", "p", "T")
MAX_PLANES = 32
LDS_LIMIT = 160 * 1024


def lds_bytes(nz: int, nx: int, itemsize: int) -> int:
    """What ``fg_plane_spectra`` declares for a plane ``[nz, nx]`` of reals of ``itemsize`` bytes: twiddles, the padded slab, two
    work buffers for each of the four waves, a flag (the same expression as ``ps_lds_bytes`` of the kernel file)."""
    c = 2 * itemsize
    nmax = max(nx, nz)
    return (nmax + nz * (nx // 2 + 1) + 8 * max(nmax, 2048 // c)) * c + 16


def check_extents(nz: int, nx: int, itemsize: Optional[int] = None, what: str = "plane spectra") -> None:
    """``ValueError`` unless ``fg_plane_spectra`` takes planes ``[nz, nx]`` (``itemsize`` None: the rules of the axes only)."""
    if nx < 8 or nx > 512 or nx & (nx - 1):
        raise ValueError(f"{what}: nx must be a power of two in 8..512, got {nx}")
    if nz != 1 and (nz < 4 or nz > 256 or nz & (nz - 1)):
        raise ValueError(f"{what}: nz must be 1 or a power of two in 4..256, got {nz}")
    if itemsize is not None and lds_bytes(nz, nx, itemsize) > LDS_LIMIT:
        raise ValueError(f"{what}: the slab of {nz} x ({nx} / 2 + 1) complex {'doubles' if itemsize == 8 else 'floats'} with its work "
                         f"buffers must fit in 160 KB of LDS, it takes {lds_bytes(nz, nx, itemsize)} bytes")


class SpectraRecord:
    """Accessors, merging, wall units and files of a record; the two accumulators below say where the sums live."""

    def __init__(self, channels: Sequence[str] = ("u", "v", "w", "p"), planes: Sequence[int] = (0,), symmetric: bool = True):
        channels = tuple(channels)
        if not channels or len(set(channels)) != len(channels) or any(c not in CHANNEL_NAMES for c in channels):
            raise ValueError(f"channels must be distinct names out of {CHANNEL_NAMES}, got {channels}")
        planes = tuple(int(p) for p in planes)
        table = len(planes) * (2 if symmetric else 1)
        if not planes or table > MAX_PLANES or min(planes) < 0:
            raise ValueError(f"planes: 1..{MAX_PLANES} non-negative row indices (mirrors included), got {planes}")
        self.channels, self.planes, self.symmetric = channels, planes, bool(symmetric)
        self.K, self.P = len(channels), len(planes)
        self.samples = 0                                   # updates taken by this accumulator (merged records add theirs)
        self.grid: Optional[tuple] = None                  # (nz, ny, nx) once known

    # ---- where the sums live: overridden by PlaneSpectra
    _count = _amp = _power = None

    def _state(self):
        if self._count is None:
            raise RuntimeError("no sample recorded yet")
        return self._count, self._amp, self._power

    def _set_state(self, count, amp, power) -> None:
        self._count, self._amp, self._power = (np.ascontiguousarray(v, np.float64) for v in (count, amp, power))

    def _unset(self) -> bool:
        return self._count is None

    def _like(self, count, amp, power, samples) -> "HostPlaneSpectra":
        r = HostPlaneSpectra(self.channels, self.planes, self.symmetric)
        r._set_state(count, amp, power)
        r.samples, r.grid = samples, self.grid
        return r

    def record(self) -> "HostPlaneSpectra":
        """A host copy of the current state."""
        return self._like(*(np.array(v) for v in self._state()), self.samples)

    def plane_table(self, ny: int) -> List[int]:
        """The rows handed to the kernel: the planes, then (``symmetric``) their mirror images ``ny - 1 - p``."""
        if max(self.planes) >= ny:
            raise ValueError(f"planes {self.planes} outside the {ny} rows of the grid")
        return list(self.planes) + ([ny - 1 - p for p in self.planes] if self.symmetric else [])

    def _take_grid(self, nz: int, ny: int, nx: int, what: str) -> None:
        if self.grid is None:
            self.grid = (nz, ny, nx)
        elif self.grid != (nz, ny, nx):
            raise ValueError(f"{what}: batch size or grid changed between updates")

    # ---- accessors
    def _ch(self, ch: Union[int, str]) -> int:
        return self.channels.index(ch) if isinstance(ch, str) else int(ch)

    @property
    def _fold(self) -> int:
        return 2 if self.symmetric else 1

    @property
    def n(self) -> int:
        """Planes averaged into every spectrum, counted the reference's way: envs x samples x (2 if symmetric)."""
        return int(round(float(self._state()[0].sum()))) * self._fold

    def _mean(self, sums: np.ndarray, ch) -> np.ndarray:
        s = sums[:, self._ch(ch)]
        if self.symmetric:
            s = s[:, :self.P] + s[:, self.P:]
        return s / (self._state()[0] * self._fold)[:, None, None, None]

    def amplitude(self, ch) -> np.ndarray:
        """Mean ``|u^(kz, kx)|`` of a channel, ``[B, P, nkz, nkx]``; the mirrored plane is folded into its plane when symmetric."""
        return self._mean(self._state()[1], ch)

    def power(self, ch) -> np.ndarray:
        """Mean ``|u^(kz, kx)|^2`` of a channel, ``[B, P, nkz, nkx]``."""
        return self._mean(self._state()[2], ch)

    # ---- merging
    def merge(self, other: "SpectraRecord") -> "SpectraRecord":
        """Add ``other``'s samples (same channels, planes, batch size and grid) to this record, env by env."""
        if (other.channels, other.planes, other.symmetric) != (self.channels, self.planes, self.symmetric):
            raise ValueError("merge: both records need the same channels, planes and symmetry")
        cB, aB, pB = other._state()
        if self._unset():
            self.grid = other.grid
            self._set_state(cB, aB, pB)
        else:
            cA, aA, pA = self._state()
            if aA.shape != aB.shape or self.grid != other.grid:
                raise ValueError(f"merge: shapes differ, {aA.shape} and {aB.shape}")
            self._set_state(cA + cB, aA + aB, pA + pB)
        self.samples += other.samples
        return self

    def pooled(self) -> "HostPlaneSpectra":
        """The envs of the batch merged into one ensemble record (``B = 1``), on the host."""
        count, amp, power = self._state()
        return self._like(count.sum(keepdims=True), amp.sum(axis=0, keepdims=True), power.sum(axis=0, keepdims=True), self.samples)

    # ---- wall units and pre-multiplied spectra (PSDOnline_Torch.get_phi)
    def _fft_sizes(self) -> List[int]:
        if self.grid is None:
            raise RuntimeError("no sample recorded yet")
        nz, _, nx = self.grid
        return [nx] if nz == 1 else [nz, nx]

    def wavelengths(self, phys_sizes, nu: float, u_wall: float) -> List[np.ndarray]:
        """``get_phi``'s wavelengths in wall units, one array per transformed axis (z then x; x alone in 2-D):
        ``1 / (k / (2 size)) / (nu / u_wall)`` for ``k = 1 .. n / 2``."""
        sizes = self._fft_sizes()
        if len(phys_sizes) != len(sizes):
            raise ValueError(f"phys_sizes must have one entry per transformed axis ({len(sizes)})")
        lstar = nu / u_wall
        return [1 / (np.arange(1, n / 2 + 0.1, 1) / (2 * size)) / lstar for n, size in zip(sizes, phys_sizes)]

    def k_grid(self, reference_layout: bool = True) -> np.ndarray:
        """The factor of the pre-multiplied spectrum, ``[nkz, nkx]``, from ``k = 1 .. n / 2`` per axis.  ``get_phi`` builds it as
        ``np.prod(np.meshgrid(kz, kx), axis=0)`` -- an array ``[nkx, nkz]`` -- and reshapes that to ``[nkz, nkx]``: the outer product
        ``kz kx`` when ``nz == nx``, a reshuffle of it otherwise.  ``reference_layout`` reproduces that; False gives the outer
        product for every shape."""
        ks = [np.arange(1, n / 2 + 0.1, 1) for n in self._fft_sizes()]
        nkz = 1 if len(ks) == 1 else len(ks[0])
        if reference_layout:
            return np.prod(np.meshgrid(*ks), axis=0).reshape(nkz, len(ks[-1]))
        return (ks[0][:, None] * ks[1][None, :]) if len(ks) == 2 else ks[0][None, :]

    def premultiplied(self, ch, phys_sizes, nu: float, u_wall: float, reference_layout: bool = True):
        """``get_phi``: (wavelengths in wall units, ``k_grid * amplitude(ch)`` ``[B, P, nkz, nkx]``)."""
        return self.wavelengths(phys_sizes, nu, u_wall), self.k_grid(reference_layout)[None, None] * self.amplitude(ch)

    # ---- files: PSDOnline_Torch.save writes <name>.json (its constructor's parameters) and <name>.npz (n, fft)
    def reference_parameters(self) -> dict:
        sizes = self._fft_sizes()
        three_d = len(sizes) == 2
        return {"total_dims": 5 if three_d else 4, "fft_dims": [2, 4] if three_d else [3], "fft_sizes": sizes, "mean_dims": [0],
                "planes": list(self.planes), "planes_dim": 3 if three_d else 2, "planes_symmetric": self.symmetric}

    def reference_fft(self) -> np.ndarray:
        """The pooled velocity amplitudes laid out as ``PSDOnline_Torch.fft``: ``[d, nkz, P, nkx]`` (2-D: ``[d, P, nkx]``)."""
        vel = [c for c in ("u", "v", "w") if c in self.channels]
        if vel[:2] != ["u", "v"]:
            raise ValueError("the reference's record is that of the velocity: channels must hold u, v(, w)")
        rec = self.pooled()
        fft = np.stack([rec.amplitude(c)[0] for c in vel])                       # [d, P, nkz, nkx]
        return fft.transpose(0, 2, 1, 3) if self.grid[0] > 1 else fft[:, :, 0]

    def save(self, path, name: str = "PSD") -> None:
        """The pooled record as ``path/name.json`` + ``path/name.npz`` for ``PSDOnline_Torch.from_file``; the npz also carries the
        sums of every channel (``amp_sum``, ``power_sum``, ``count``, ``samples``, ``channels``, ``grid``), which ``load`` reads."""
        rec = self.pooled()
        count, amp, power = rec._state()
        os.makedirs(str(path), exist_ok=True)
        with open(os.path.join(str(path), name + ".json"), "w") as f:
            json.dump(self.reference_parameters(), f)
        np.savez_compressed(os.path.join(str(path), name + ".npz"), n=np.asarray(self.n), fft=self.reference_fft(), amp_sum=amp,
                            power_sum=power, count=count, samples=np.asarray(self.samples), channels=np.array(self.channels),
                            grid=np.asarray(self.grid))

    @staticmethod
    def load(path, name: str = "PSD") -> "HostPlaneSpectra":
        """The pooled record ``save`` wrote, bit for bit."""
        with open(os.path.join(str(path), name + ".json")) as f:
            params = json.load(f)
        with np.load(os.path.join(str(path), name + ".npz")) as z:
            r = HostPlaneSpectra(tuple(str(c) for c in z["channels"]), params["planes"], params["planes_symmetric"])
            r._set_state(z["count"], z["amp_sum"], z["power_sum"])
            r.samples, r.grid = int(z["samples"]), tuple(int(v) for v in z["grid"])
        return r


class HostPlaneSpectra(SpectraRecord):
    """The NumPy fp64 twin of ``PlaneSpectra``: same interface and arithmetic with ``numpy.fft``, arrays on the host."""

    def update(self, velocity, pressure=None, scalar=None) -> None:
        what = "HostPlaneSpectra.update"
        velocity = np.asarray(velocity)
        pressure, scalar = (None if t is None else np.asarray(t) for t in (pressure, scalar))
        fields = [np.asarray(t[:, c], np.float64) for t, c in _gather(self.channels, velocity, pressure, scalar, what)]
        v = np.stack(fields, axis=1)                                              # [B, K, (Z,) Y, X]
        if v.ndim == 4:
            v = v[:, :, None]
        B, _, nz, ny, nx = v.shape
        check_extents(nz, nx, None, what)
        if not self._unset() and self._amp.shape[0] != B:
            raise ValueError(f"{what}: batch size or grid changed between updates")
        self._take_grid(nz, ny, nx, what)
        sel = np.moveaxis(v[:, :, :, self.plane_table(ny)], 3, 2)                 # [B, K, T, nz, nx]
        with np.errstate(all="ignore"):
            spec = np.fft.fftn(sel, axes=(3, 4))[..., :max(nz // 2, 1), :nx // 2]
            amp = np.abs(spec)
            power = spec.real ** 2 + spec.imag ** 2
        bad = ~np.isfinite(sel).all(axis=(3, 4))                                  # a non-finite cell: every mode of its slab is NaN
        amp[bad] = np.nan
        power[bad] = np.nan
        if self._unset():
            self._set_state(np.ones(B), amp, power)
        else:
            self._set_state(self._count + 1.0, self._amp + amp, self._power + power)
        self.samples += 1


class PlaneSpectra(F.DeviceState, SpectraRecord):
    """The GPU accumulator.  ``update(velocity, pressure, scalar=None)`` takes the domain's own tensors (``[B, d, (Z,) Y, X]``,
    ``[B, 1, ...]``, ``[B, S, ...]``; float32 -> ``libfluidgym_hip.so``, float64 -> the fp64 library), reads their component slices in
    place and runs one launch on the current stream; nothing comes back to the host until an accessor is called."""

    _merge_into = "a HostPlaneSpectra"
    # _dev: (amp, power) [B, K, T, nkz, nkx] on the device
    _counts = None         # [B] on the host: the kernel keeps sums, the samples are counted here

    def _state(self):
        return (self._counts,) + self._read(2)

    def _set_state(self, count, amp, power) -> None:
        self._write(amp, power)
        self._counts = np.ascontiguousarray(count, np.float64)

    def update(self, velocity: torch.Tensor, pressure: Optional[torch.Tensor] = None, scalar: Optional[torch.Tensor] = None) -> None:
        what = "PlaneSpectra.update"
        used = (velocity,) + ((pressure,) if "p" in self.channels else ()) + ((scalar,) if "T" in self.channels else ())
        F.check_device_fields(used, what, "HostPlaneSpectra")
        parts = [(t.contiguous(), c) for t, c in _gather(self.channels, velocity, pressure, scalar, what)]
        B, nz, ny, nx = F.grid_of(velocity)
        check_extents(nz, nx, velocity.element_size(), what)
        table = self.plane_table(ny)
        dev = velocity.device
        if self._dev is None:
            self._take_grid(nz, ny, nx, what)
            self._shape = (B, nz, ny, nx, dev)
            shape = (B, self.K, len(table), max(nz // 2, 1), nx // 2)
            self._dev = (torch.zeros(shape, dtype=torch.float64, device=dev), torch.zeros(shape, dtype=torch.float64, device=dev))
            self._counts = np.zeros(B)
        elif self._shape != (B, nz, ny, nx, dev):
            raise ValueError(f"{what}: batch size, grid or device changed between updates")
        ptrs, strides = F.channel_table(parts, nz * ny * nx)
        rows = (ctypes.c_int32 * len(table))(*table)
        lib = F.library(velocity.dtype)
        amp, power = self._dev
        with torch.cuda.device(dev):
            L.check(lib.fg_plane_spectra(ptrs, strides, self.K, B, nz, ny, nx, rows, len(table), F.ptr(amp), F.ptr(power),
                                         F.stream_ptr(dev)), lib=lib)
        self._counts = self._counts + 1.0
        self.samples += 1
