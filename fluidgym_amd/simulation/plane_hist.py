"""Online PDFs and joint PDFs of wall-parallel planes: per listed wall-normal row the histogram of each channel over the
homogeneous directions ``z, x`` and the joint histogram of chosen channel pairs, summed over the samples of a run.

The reference records moments, spectra, budgets and correlations of the planes (``VelocityStats``) and no distribution; this
recorder has no counterpart there.  One sample of a batch of ``B`` envs is one launch of ``fg_plane_histogram``
(``csrc/fg_planehist.hip``) that leaves nothing on the host.

Bin rule (the kernel's, and ``bin_slots`` here): in the field's dtype, with two separately rounded operations,
``t = (v - lo) * scale`` with ``scale = bins / (hi - lo)`` formed in fp64 and rounded to the dtype once; slot ``bins + 2`` for NaN,
``0`` for ``!(t >= 0)`` (below), ``bins + 1`` for ``t >= bins`` (at or above ``hi``), ``1 + int(t)`` otherwise.  ``edges`` are the
nominal fp64 edges ``lo + i (hi - lo) / bins``; a value within rounding of an edge may sit in the neighbouring bin.  A pair
``(a, b)`` is binned on ``joint_bins`` coarsened bins per axis, index ``(slot - 1) // (bins // joint_bins)``, when both slots are
in range, and counted as "outside" otherwise: the joint table's marginals are the coarsened 1-D counts of the cells in range in
both channels.

A record holds ``counts [B, R, K, bins + 3]`` and ``joint [B, R, P, joint_bins^2 + 1]`` (``uint64``), the number of samples and the
tables.  Records merge by addition.  ``save`` writes one ``.npz`` (no reference layout exists) with the keys ``counts``, ``joint``,
``n_samples``, ``channels``, ``pairs`` (``[P, 2]`` channel indices), ``bins``, ``joint_bins``, ``rows``, ``lo``, ``hi`` (fp64
``[R, K]``), ``scale`` and ``lo_real`` (the rounded tables the bins were taken with) and ``cells`` (``nz nx``).

``PlaneHistograms`` accumulates on the GPU, ``HostPlaneHistograms`` is its NumPy twin with the same accessors.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from .. import _lib as L
from . import plane_fields as F

CHANNEL_ORDER = ("u", "v", "w", "p", "T")
MAX_BINS, MAX_JOINT_BINS, MAX_PAIRS = 256, 64, 6


def bin_slots(v: np.ndarray, lo, scale, bins: int) -> np.ndarray:
    """Slots ``0 .. bins + 2`` of ``v`` by the bin rule, in ``v``'s dtype (``lo`` and ``scale`` broadcast against ``v``)."""
    dt = v.dtype.type
    with np.errstate(all="ignore"):
        d = np.subtract(v, np.asarray(lo, v.dtype), dtype=v.dtype)
        t = np.multiply(d, np.asarray(scale, v.dtype), dtype=v.dtype)
        inside = (t >= dt(0)) & (t < dt(bins))
        slot = np.where(inside, 1 + np.where(inside, t, 0).astype(np.int64), 0)
        slot = np.where(t >= dt(bins), bins + 1, slot)
    return np.where(np.isnan(v), bins + 2, slot)


def sample_histograms(values: np.ndarray, rows, lo, scale, bins: int, pairs, joint_bins: int):
    """One sample on the host: ``values [K, B, nz, ny, nx]`` -> ``counts [B, R, K, bins + 3]``, ``joint [B, R, P, jb^2 + 1]``."""
    K, B = values.shape[:2]
    R, P, ratio, J = len(rows), len(pairs), bins // joint_bins, joint_bins * joint_bins
    v = values[:, :, :, np.asarray(rows, np.int64), :]                                   # [K, B, nz, R, nx]
    slot = np.stack([bin_slots(v[k], lo[None, None, :, k, None], scale[None, None, :, k, None], bins) for k in range(K)])
    slot = np.moveaxis(slot, 3, 2).reshape(K, B, R, -1)                                  # [K, B, R, cells]
    counts = np.zeros((B, R, K, bins + 3), np.uint64)
    joint = np.zeros((B, R, P, J + 1), np.uint64)
    for b in range(B):
        for r in range(R):
            for k in range(K):
                counts[b, r, k] = np.bincount(slot[k, b, r], minlength=bins + 3)
            for p, (ia, ib) in enumerate(pairs):
                sa, sb = slot[ia, b, r], slot[ib, b, r]
                inside = (sa >= 1) & (sa <= bins) & (sb >= 1) & (sb <= bins)
                cell = np.where(inside, (sa - 1) // ratio * joint_bins + (sb - 1) // ratio, J)
                joint[b, r, p] = np.bincount(cell, minlength=J + 1)
    return counts, joint


class HistogramRecord:
    """Tables, accessors, merging and files of a record; the two accumulators below say where the counters live."""

    def __init__(self, channels: Sequence[str], ranges: Dict[str, object], bins: int = 128, joint: Sequence[Tuple[str, str]] = (),
                 joint_bins: int = 32, rows: Optional[Sequence[int]] = None):
        channels = tuple(channels)
        order = [CHANNEL_ORDER.index(c) for c in channels if c in CHANNEL_ORDER]
        if not channels or len(order) != len(channels) or order != sorted(set(order)):
            raise ValueError(f"channels must be names from {CHANNEL_ORDER}, each once and in that order, got {channels}")
        bins, joint_bins = int(bins), int(joint_bins)
        if not 2 <= bins <= MAX_BINS:
            raise ValueError(f"bins must be 2..{MAX_BINS}, got {bins}")
        if not 2 <= joint_bins <= MAX_JOINT_BINS or bins % joint_bins:
            raise ValueError(f"joint_bins must be 2..{MAX_JOINT_BINS} and divide bins = {bins}, got {joint_bins}")
        joint = tuple(tuple(p) for p in joint)
        if len(joint) > MAX_PAIRS:
            raise ValueError(f"at most {MAX_PAIRS} joint pairs, got {len(joint)}")
        for p in joint:
            if len(p) != 2 or p[0] not in channels or p[1] not in channels:
                raise ValueError(f"joint pair {p}: two names from the channels {channels}")
        if len(set(joint)) != len(joint):
            raise ValueError(f"joint pairs must differ, got {joint}")
        if not isinstance(ranges, dict) or set(ranges) != set(channels):
            raise ValueError(f"ranges needs one entry per channel {channels}")
        self.channels, self.bins, self.joint, self.joint_bins = channels, bins, joint, joint_bins
        self.K, self.P = len(channels), len(joint)
        self.pairs = [(channels.index(a), channels.index(b)) for a, b in joint]
        self._ranges = {}
        for c in channels:
            rg = np.asarray(ranges[c], np.float64)
            if rg.shape != (2,) and not (rg.ndim == 2 and rg.shape[1] == 2 and rg.shape[0] >= 1):
                raise ValueError(f"ranges[{c!r}] must be (lo, hi) or an array [n_rows, 2], got shape {rg.shape}")
            if not np.isfinite(rg).all() or not (rg[..., 1] > rg[..., 0]).all():
                raise ValueError(f"ranges[{c!r}]: finite edges with hi > lo")
            self._ranges[c] = rg
        self.rows = None
        if rows is not None:
            rows = np.asarray(list(rows), np.int64)
            if rows.ndim != 1 or len(rows) < 1 or (rows < 0).any() or (np.diff(rows) <= 0).any():
                raise ValueError(f"rows must be ascending, unique and non-negative, got {rows.tolist()}")
            self._set_rows(rows)
        self.lo = self.hi = self.lo_real = self.scale = None
        self.cells = None
        self.n_samples = 0

    def _set_rows(self, rows: np.ndarray) -> None:
        for c, rg in self._ranges.items():
            if rg.ndim == 2 and rg.shape[0] != len(rows):
                raise ValueError(f"ranges[{c!r}] has {rg.shape[0]} rows, {len(rows)} rows are listed")
        self.rows = rows.astype(np.int32)

    def _resolve(self, nz: int, ny: int, nx: int, dtype) -> None:
        """The tables for a grid and a field dtype: at the first update."""
        if self.rows is None:
            self._set_rows(np.arange(ny))
        if self.rows[-1] >= ny:
            raise ValueError(f"row {int(self.rows[-1])} is outside the grid's {ny} rows")
        if nz * nx > 2 ** 30:
            raise ValueError("a plane of more than 2^30 cells")
        R = len(self.rows)
        rg = np.stack([np.broadcast_to(self._ranges[c], (R, 2)) for c in self.channels], axis=1)     # [R, K, 2]
        self.lo, self.hi = rg[..., 0].copy(), rg[..., 1].copy()
        with np.errstate(over="ignore"):
            self.lo_real = self.lo.astype(dtype)
            self.scale = (self.bins / (self.hi - self.lo)).astype(dtype)
        if not np.isfinite(self.scale).all() or not np.isfinite(self.lo_real).all():
            raise ValueError(f"the ranges do not fit {np.dtype(dtype).name}")
        self.cells = int(nz * nx)

    # ---- where the counters live: overridden by PlaneHistograms
    _counts = _joint = None

    def _state(self):
        if self._counts is None:
            raise RuntimeError("no sample recorded yet")
        return self._counts, self._joint

    def _set_state(self, counts, joint) -> None:
        self._counts, self._joint = np.ascontiguousarray(counts, np.uint64), np.ascontiguousarray(joint, np.uint64)

    def _unset(self) -> bool:
        return self._counts is None

    def _like(self, counts, joint, n_samples) -> "HostPlaneHistograms":
        r = HostPlaneHistograms(self.channels, {c: (0.0, 1.0) for c in self.channels}, self.bins, self.joint, self.joint_bins)
        r._ranges = dict(self._ranges)
        r.rows, r.lo, r.hi, r.lo_real, r.scale, r.cells = self.rows, self.lo, self.hi, self.lo_real, self.scale, self.cells
        r._set_state(counts, joint)
        r.n_samples = int(n_samples)
        return r

    def record(self) -> "HostPlaneHistograms":
        """A host copy of the current state."""
        c, j = self._state()
        return self._like(np.array(c), np.array(j), self.n_samples)

    # ---- 1-D accessors
    def _ch(self, ch: Union[int, str]) -> int:
        return self.channels.index(ch) if isinstance(ch, str) else int(ch)

    def _need_tables(self):
        if self.lo is None:
            raise RuntimeError("no sample recorded yet")

    def counts(self, ch) -> np.ndarray:
        """Cells per bin, ``[B, R, bins]``."""
        return np.array(self._state()[0][:, :, self._ch(ch), 1:self.bins + 1])

    def below(self, ch) -> np.ndarray:
        return np.array(self._state()[0][:, :, self._ch(ch), 0])

    def above(self, ch) -> np.ndarray:
        return np.array(self._state()[0][:, :, self._ch(ch), self.bins + 1])

    def nonfinite(self, ch) -> np.ndarray:
        """NaN cells, ``[B, R]`` (``-inf`` counts as below, ``+inf`` as above)."""
        return np.array(self._state()[0][:, :, self._ch(ch), self.bins + 2])

    def width(self, ch) -> np.ndarray:
        """Bin width per listed row, ``[R]``."""
        self._need_tables()
        k = self._ch(ch)
        return (self.hi[:, k] - self.lo[:, k]) / self.bins

    def edges(self, ch) -> np.ndarray:
        """Nominal bin edges per listed row, ``[R, bins + 1]``."""
        self._need_tables()
        k = self._ch(ch)
        return self.lo[:, k, None] + (self.hi[:, k] - self.lo[:, k])[:, None] * (np.arange(self.bins + 1) / self.bins)

    def centers(self, ch) -> np.ndarray:
        e = self.edges(ch)
        return 0.5 * (e[:, 1:] + e[:, :-1])

    def pdf(self, ch) -> np.ndarray:
        """Density over the in-range cells, ``[B, R, bins]``: integrates to 1 over ``[lo, hi]`` (NaN where no cell is in range)."""
        c = self.counts(ch).astype(np.float64)
        with np.errstate(all="ignore"):
            return c / (c.sum(axis=-1, keepdims=True) * self.width(ch)[None, :, None])

    def cdf(self, ch) -> np.ndarray:
        """Share of the in-range cells below each bin's upper edge, ``[B, R, bins]``."""
        c = self.counts(ch).astype(np.float64)
        with np.errstate(all="ignore"):
            return np.cumsum(c, axis=-1) / c.sum(axis=-1, keepdims=True)

    def quantile(self, ch, q) -> np.ndarray:
        """The value below which a share ``q`` of the in-range cells lies, linear inside a bin: ``[B, R]`` for a scalar ``q``,
        ``[B, R, len(q)]`` for a sequence."""
        qs = np.atleast_1d(np.asarray(q, np.float64))
        if ((qs < 0) | (qs > 1)).any():
            raise ValueError("quantile: q in [0, 1]")
        c = self.counts(ch).astype(np.float64)
        cum = np.cumsum(c, axis=-1)
        total = cum[..., -1:]
        e, w = self.edges(ch), self.width(ch)
        out = np.empty(c.shape[:2] + (len(qs),))
        for i, qi in enumerate(qs):
            target = qi * total                                                          # [B, R, 1]
            idx = np.minimum((cum < target).sum(axis=-1), self.bins - 1)                 # first bin whose cumulative count reaches it
            before = np.take_along_axis(cum, idx[..., None], -1)[..., 0] - np.take_along_axis(c, idx[..., None], -1)[..., 0]
            inbin = np.take_along_axis(c, idx[..., None], -1)[..., 0]
            with np.errstate(all="ignore"):
                frac = np.where(inbin > 0, (target[..., 0] - before) / inbin, 0.0)
            out[..., i] = np.take_along_axis(np.broadcast_to(e[None], c.shape[:2] + (self.bins + 1,)), idx[..., None], -1)[..., 0] \
                + frac * w[None]
            out[..., i] = np.where(total[..., 0] > 0, out[..., i], np.nan)
        return out[..., 0] if np.ndim(q) == 0 else out

    def mean(self, ch) -> np.ndarray:
        """Mean of the in-range cells from bin centres, ``[B, R]``."""
        c = self.counts(ch).astype(np.float64)
        with np.errstate(all="ignore"):
            return (c * self.centers(ch)[None]).sum(axis=-1) / c.sum(axis=-1)

    def variance(self, ch) -> np.ndarray:
        c = self.counts(ch).astype(np.float64)
        with np.errstate(all="ignore"):
            d = self.centers(ch)[None] - self.mean(ch)[..., None]
            return (c * d * d).sum(axis=-1) / c.sum(axis=-1)

    # ---- joint accessors
    def _pair(self, a, b) -> int:
        key = (self.channels[self._ch(a)], self.channels[self._ch(b)])
        if key not in self.joint:
            raise KeyError(f"the pair {key} is not recorded (joint = {self.joint})")
        return self.joint.index(key)

    def joint_counts(self, a, b) -> np.ndarray:
        """Cells per joint bin, ``[B, R, joint_bins, joint_bins]`` (``a`` along the first bin axis)."""
        j = self._state()[1][:, :, self._pair(a, b), :-1]
        return np.array(j).reshape(j.shape[:2] + (self.joint_bins, self.joint_bins))

    def joint_outside(self, a, b) -> np.ndarray:
        """Cells out of range (or NaN) in either channel, ``[B, R]``."""
        return np.array(self._state()[1][:, :, self._pair(a, b), -1])

    def joint_centers(self, ch) -> np.ndarray:
        """Centres of the coarsened bins of a channel, ``[R, joint_bins]``."""
        e = self.edges(ch)[:, ::self.bins // self.joint_bins]
        return 0.5 * (e[:, 1:] + e[:, :-1])

    def joint_pdf(self, a, b) -> np.ndarray:
        """Joint density over the cells in range in both channels, ``[B, R, joint_bins, joint_bins]``."""
        c = self.joint_counts(a, b).astype(np.float64)
        ratio = self.bins // self.joint_bins
        area = (self.width(a) * ratio) * (self.width(b) * ratio)
        with np.errstate(all="ignore"):
            return c / (c.sum(axis=(-1, -2), keepdims=True) * area[None, :, None, None])

    def quadrants(self, a, b, mean_a=None, mean_b=None, hole: float = 0.0) -> Dict[str, np.ndarray]:
        """Quadrant split of the joint table of ``(a, b)`` at the centres of its bins.  With ``a' = a - mean_a``,
        ``b' = b - mean_b`` (the means default to those of the joint table itself; scalars or ``[B, R]``) the classes are Q1
        (``a' > 0, b' > 0``), Q2 (``a' < 0, b' > 0``: ejections of ``(u, v)``), Q3 (``a' < 0, b' < 0``), Q4 (``a' > 0, b' < 0``:
        sweeps) and the hole ``|a' b'| <= hole * rms_a * rms_b`` (rms about the means, from the joint table), which at ``hole = 0``
        holds the cells with ``a' b' = 0``.  Returns ``share [B, R, 5]``, the share of the in-range cells per class, and
        ``contribution [B, R, 5]``, each class's part of ``<a' b'>``; both sum to the whole over the five classes."""
        c = self.joint_counts(a, b).astype(np.float64)
        ca, cb = self.joint_centers(a)[None, :, :, None], self.joint_centers(b)[None, :, None, :]
        with np.errstate(all="ignore"):
            total = c.sum(axis=(-1, -2))
            ma = (c * ca).sum(axis=(-1, -2)) / total if mean_a is None else np.broadcast_to(np.asarray(mean_a, np.float64), total.shape)
            mb = (c * cb).sum(axis=(-1, -2)) / total if mean_b is None else np.broadcast_to(np.asarray(mean_b, np.float64), total.shape)
            da, db = ca - ma[..., None, None], cb - mb[..., None, None]
            rms_a = np.sqrt((c * da * da).sum(axis=(-1, -2)) / total)
            rms_b = np.sqrt((c * db * db).sum(axis=(-1, -2)) / total)
            prod = da * db
            in_hole = np.abs(prod) <= (float(hole) * rms_a * rms_b)[..., None, None]
            classes = [(da > 0) & (db > 0), (da < 0) & (db > 0), (da < 0) & (db < 0), (da > 0) & (db < 0)]
            classes = [m & ~in_hole for m in classes] + [in_hole]
            share = np.stack([(c * m).sum(axis=(-1, -2)) / total for m in classes], axis=-1)
            contribution = np.stack([(c * m * prod).sum(axis=(-1, -2)) / total for m in classes], axis=-1)
        return {"share": share, "contribution": contribution}

    # ---- merging
    def _same_tables(self, other: "HistogramRecord") -> bool:
        if (self.channels, self.bins, self.joint, self.joint_bins) != (other.channels, other.bins, other.joint, other.joint_bins):
            return False
        mine, theirs = (self.rows, self.lo, self.hi, self.lo_real, self.scale), (other.rows, other.lo, other.hi, other.lo_real, other.scale)
        return self.cells == other.cells and all(
            a is not None and b is not None and a.dtype == b.dtype and np.array_equal(a, b) for a, b in zip(mine, theirs))

    def merge(self, other: "HistogramRecord") -> "HistogramRecord":
        """Add ``other``'s samples to this record, env by env: an addition of counters.  Both need the same tables."""
        oc, oj = other._state()
        if self._unset():
            if (self.channels, self.bins, self.joint, self.joint_bins) != (other.channels, other.bins, other.joint, other.joint_bins):
                raise ValueError("merge: both records need the same channels, bins, pairs and joint_bins")
            self._adopt(other, oc, oj)
            return self
        if not self._same_tables(other):
            raise ValueError("merge: both records need the same channels, bins, pairs, rows, ranges, dtype and plane size")
        c, j = self._state()
        if c.shape != oc.shape:
            raise ValueError(f"merge: batch sizes differ, {c.shape[0]} and {oc.shape[0]}")
        self._set_state(c + oc, j + oj)
        self.n_samples += other.n_samples
        return self

    def _adopt(self, other, counts, joint) -> None:
        self._ranges = dict(other._ranges)
        self.rows, self.lo, self.hi, self.lo_real, self.scale, self.cells = (other.rows, other.lo, other.hi, other.lo_real, other.scale,
                                                                              other.cells)
        self._set_state(np.array(counts), np.array(joint))
        self.n_samples = other.n_samples

    def pooled(self) -> "HostPlaneHistograms":
        """The envs of the batch summed into one ensemble record (``B = 1``)."""
        c, j = self._state()
        return self._like(c.sum(axis=0, keepdims=True, dtype=np.uint64), j.sum(axis=0, keepdims=True, dtype=np.uint64), self.n_samples)

    # ---- files
    def save(self, path) -> None:
        """One ``.npz`` with the counters and the tables (keys in the module's docstring)."""
        c, j = self._state()
        np.savez_compressed(path, counts=c, joint=j, n_samples=np.int64(self.n_samples), channels=np.array(self.channels),
                            pairs=np.asarray(self.pairs, np.int32).reshape(-1, 2), bins=np.int32(self.bins),
                            joint_bins=np.int32(self.joint_bins), rows=self.rows, lo=self.lo, hi=self.hi, scale=self.scale,
                            lo_real=self.lo_real, cells=np.int64(self.cells))

    @staticmethod
    def load(path) -> "HostPlaneHistograms":
        """The record ``save`` wrote, bit for bit."""
        with np.load(path) as z:
            channels = tuple(str(c) for c in z["channels"])
            joint = tuple((channels[a], channels[b]) for a, b in z["pairs"])
            lo, hi = z["lo"], z["hi"]
            r = HostPlaneHistograms(channels, {c: np.stack([lo[:, k], hi[:, k]], axis=1) for k, c in enumerate(channels)},
                                    int(z["bins"]), joint, int(z["joint_bins"]), rows=z["rows"].tolist())
            r.lo, r.hi, r.lo_real, r.scale, r.cells = lo, hi, z["lo_real"], z["scale"], int(z["cells"])
            r._set_state(z["counts"], z["joint"])
            r.n_samples = int(z["n_samples"])
        return r


def _fields(channels, velocity, pressure, scalar, what: str):
    return F.gather(channels, velocity, pressure, scalar, what)


class HostPlaneHistograms(HistogramRecord):
    """The NumPy twin of ``PlaneHistograms``: same interface, same bin rule in the arrays' dtype, counters on the host."""

    def update(self, velocity, pressure=None, scalar=None) -> None:
        what = "HostPlaneHistograms.update"
        velocity = np.asarray(velocity)
        pressure, scalar = (None if t is None else np.asarray(t) for t in (pressure, scalar))
        if velocity.dtype not in (np.float32, np.float64):
            raise TypeError(f"{what}: float32 or float64 fields, got {velocity.dtype}")
        parts = _fields(self.channels, velocity, pressure, scalar, what)
        if any(t.dtype != velocity.dtype for t, _ in parts):
            raise TypeError(f"{what}: all fields need one dtype")
        v = np.stack([t[:, c] for t, c in parts])                      # [K, B, (Z,) Y, X]
        if v.ndim == 4:
            v = v[:, :, None]
        B, nz, ny, nx = v.shape[1:]
        if self.lo is None:
            self._resolve(nz, ny, nx, v.dtype)
        elif self.scale.dtype != v.dtype or self.cells != nz * nx or self.rows[-1] >= ny:
            raise ValueError(f"{what}: dtype or grid changed between updates")
        counts, joint = sample_histograms(v, self.rows, self.lo_real, self.scale, self.bins, self.pairs, self.joint_bins)
        if self._counts is None:
            self._set_state(counts, joint)
        elif self._counts.shape != counts.shape:
            raise ValueError(f"{what}: batch size changed between updates")
        else:
            self._set_state(self._counts + counts, self._joint + joint)
        self.n_samples += 1


class PlaneHistograms(HistogramRecord):
    """The GPU accumulator.  ``update(velocity, pressure=None, scalar=None)`` takes the domain's own tensors (``[B, d, (Z,) Y, X]``,
    ``[B, 1, ...]``, ``[B, S, ...]``; float32 -> ``libfluidgym_hip.so``, float64 -> the fp64 library), reads their component slices in
    place and runs on the current stream; nothing comes back to the host until an accessor is called."""

    _dev = None         # (counts [B, R, K, bins + 3], joint [B, R, P, jb^2 + 1]) as int64 tensors holding the uint64 bits; lo, scale
    _shape = None

    def _unset(self) -> bool:
        return self._dev is None

    def _state(self):
        if self._dev is None:
            raise RuntimeError("no sample recorded yet")
        return tuple(t.cpu().numpy().view(np.uint64) for t in self._dev[:2])

    def _set_state(self, counts, joint) -> None:
        if self._dev is None:
            raise RuntimeError("PlaneHistograms takes a state only after its first update (merge into a HostPlaneHistograms instead)")
        for t, v in zip(self._dev, (counts, joint)):
            t.copy_(torch.from_numpy(np.ascontiguousarray(v, np.uint64).view(np.int64)).reshape(t.shape))

    def _adopt(self, other, counts, joint) -> None:
        raise RuntimeError("PlaneHistograms takes a state only after its first update (merge into a HostPlaneHistograms instead)")

    def update(self, velocity: torch.Tensor, pressure: Optional[torch.Tensor] = None, scalar: Optional[torch.Tensor] = None) -> None:
        what = "PlaneHistograms.update"
        used = (velocity,) + ((pressure,) if "p" in self.channels else ()) + ((scalar,) if "T" in self.channels else ())
        F.check_device_fields(used, what, "HostPlaneHistograms")
        parts = [(t.contiguous(), c) for t, c in _fields(self.channels, velocity, pressure, scalar, what)]
        B, nz, ny, nx = F.grid_of(velocity)
        dev = velocity.device
        if self._dev is None:
            self._resolve(nz, ny, nx, np.float64 if velocity.dtype == torch.float64 else np.float32)
            if B * len(self.rows) > 2 ** 31 - 1:
                raise ValueError(f"{what}: batch * rows too large for one launch")
            R = len(self.rows)
            self._shape = (B, nz, ny, nx, dev, velocity.dtype)
            self._dev = (torch.zeros(B, R, self.K, self.bins + 3, dtype=torch.int64, device=dev),
                         torch.zeros(B, R, self.P, self.joint_bins ** 2 + 1, dtype=torch.int64, device=dev),
                         torch.from_numpy(self.lo_real).to(dev), torch.from_numpy(self.scale).to(dev))
            self._rows_c = (ctypes.c_int32 * R)(*self.rows.tolist())
            self._pairs_c = (ctypes.c_int32 * max(2 * self.P, 1))(*[i for p in self.pairs for i in p])
        elif self._shape != (B, nz, ny, nx, dev, velocity.dtype):
            raise ValueError(f"{what}: batch size, grid, dtype or device changed between updates")
        ptrs, strides = F.channel_table(parts, nz * ny * nx)
        lib = F.library(velocity.dtype)
        counts, joint, lo, scale = self._dev
        with torch.cuda.device(dev):
            L.check(lib.fg_plane_histogram(ptrs, strides, self.K, B, nz, ny, nx, self._rows_c, len(self.rows), F.ptr(lo), F.ptr(scale),
                                           self.bins, self._pairs_c, self.P, self.joint_bins, F.ptr(counts),
                                           F.ptr(joint) if self.P else None, F.stream_ptr(dev)), lib=lib)
        self.n_samples += 1
