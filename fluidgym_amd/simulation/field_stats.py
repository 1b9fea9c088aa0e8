"""Running summaries of device fields: the ``Stats`` of velocity magnitude and pressure in ``domain_statistics.json``.

The reference ships one ``Stats`` record (mean, min, max, p5 .. p95) per env type for velocity magnitude and pressure over an
uncontrolled rollout; its generator is not part of its package.  The definition here is this project's own: every cell of every
sample counts once (no volume weights) -- what ``tensor.mean()`` / ``quantile`` over the stacked fields would give.

A sample is summarised on the device by ``fg_field_summary`` (``csrc/fg_fieldstats.hip``): exact min / max / sum / counts per
env, and a histogram per env over uniform bins ``[lo + k * width, lo + (k + 1) * width)``.  The samples of a rollout are not
known in advance, so the bin range GROWS: when a sample's min or max falls outside, ``width`` is doubled until it fits, by
merging adjacent bin pairs into one half of the array -- integer additions, so no count is lost or split.  ``width`` is a power
of two and ``lo`` a multiple of it, so every edge is exact in fp64 and the folded counts equal a fresh histogram of the pooled
data over the final range.  Quantiles are read
from the pooled histogram with linear interpolation inside the bin: their error is bounded by one final bin width.

``HistogramRange`` holds the range arithmetic for both ``FieldSummary`` (device) and ``HostFieldSummary`` (its NumPy twin, used
by the tests as the reference and usable where the data already lives on the host).
"""
from __future__ import annotations

import ctypes
import math
from typing import List, Optional, Sequence, Union

import numpy as np
import torch

from .. import _lib as L
from ..types import Stats

QUANTILES = (0.05, 0.25, 0.50, 0.75, 0.95)     # p5, p25, p50, p75, p95 of Stats
MAX_BINS = 4096


def bin_index(values: np.ndarray, lo: float, width: float, nbins: int) -> np.ndarray:
    """The bin of every (finite) value: the fp64 expression the kernel evaluates."""
    q = np.floor((np.asarray(values, np.float64) - np.float64(lo)) / np.float64(width))
    return np.clip(q, 0, nbins - 1).astype(np.int64)


class HistogramRange:
    """``nbins`` uniform bins over ``[lo, lo + nbins * width)``; ``cover`` widens it and says how to fold the counts."""

    def __init__(self, nbins: int):
        if not (2 <= int(nbins) <= MAX_BINS) or int(nbins) % 2:
            raise ValueError(f"nbins must be an even number in 2..{MAX_BINS}, got {nbins}")
        self.nbins = int(nbins)
        self.lo: Optional[float] = None
        self.width: Optional[float] = None

    @property
    def hi(self) -> float:
        return self.lo + self.nbins * self.width

    def start(self, vmin: float, vmax: float, magnitude: bool) -> None:
        """The first sample sets the range: ``lo = min`` (0 for a magnitude) and ``width = (max - lo) / nbins``, both snapped to
        a dyadic grid -- ``width`` up to the next power of two, ``lo`` down to a multiple of it.  Every bin edge, now and after
        any number of doublings, is then an exactly representable number, so counts folded by ``cover`` are the counts a fresh
        histogram over the final range gives (with ``lo = min`` taken literally the first minimum sits ON an edge that later
        moves by a rounding error).  A constant field gets a positive width of the scale of its value."""
        lo = 0.0 if magnitude else float(vmin)
        raw = (float(vmax) - lo) / self.nbins
        if not raw > 0.0:
            raw = max(abs(float(vmax)), 1.0) / self.nbins
        m, e = math.frexp(max(raw, 2.0 ** -900))
        self.width = math.ldexp(1.0, e - 1 if m == 0.5 else e)
        self.lo = math.floor(lo / self.width) * self.width
        self.cover(vmin, vmax)

    def cover(self, vmin: float, vmax: float, width: float = 0.0) -> List[str]:
        """Double ``width`` until ``[vmin, vmax]`` lies inside ``[lo, hi)`` (and ``width`` is at least the one given); returns
        the folds to apply to the counts, in order: "up" keeps ``lo`` (pairs merge into the lower half), "down" moves ``lo``
        down by the old span (pairs merge into the upper half)."""
        folds = []
        while vmax >= self.hi or self.width < width:
            self.width *= 2.0
            folds.append("up")
        while vmin < self.lo:
            self.lo -= self.nbins * self.width
            self.width *= 2.0
            folds.append("down")
        return folds

    @staticmethod
    def fold(hist, direction: str):
        """Merge adjacent bin pairs of ``hist [..., nbins]`` (NumPy or torch, integer) into one half; the other half is zero."""
        pairs = hist[..., 0::2] + hist[..., 1::2]
        out = hist * 0
        half = hist.shape[-1] // 2
        if direction == "up":
            out[..., :half] = pairs
        else:
            out[..., half:] = pairs
        return out


def stats_from_histogram(counts: np.ndarray, lo: float, width: float, total: float, vmin: float, vmax: float) -> Stats:
    """``Stats`` of ``counts [nbins]`` (int64) with the exact ``total`` (sum of the values), ``vmin``, ``vmax``.  Percentile q is
    the point below which q * N of the mass lies when a bin's counts are spread evenly over it, clipped to [vmin, vmax]."""
    counts = np.asarray(counts, np.int64)
    n = int(counts.sum())
    if n == 0:
        nan = float("nan")
        return Stats(*([nan] * 8))
    cum = np.cumsum(counts)
    out = []
    for q in QUANTILES:
        target = q * n
        k = int(np.searchsorted(cum, target, side="left"))
        k = min(k, counts.size - 1)
        below = float(cum[k] - counts[k])
        frac = (target - below) / float(counts[k]) if counts[k] else 0.0
        out.append(float(min(max(lo + (k + frac) * width, vmin), vmax)))
    return Stats(float(total) / n, float(vmin), float(vmax), *out)


class _Moments:
    """Exact running min / max / sum / counts, per env."""

    def __init__(self):
        self.min = self.max = self.sum = self.count = self.nonfinite = None

    def add(self, mn, mx, sm, cnt, bad) -> None:
        if self.count is None:
            B = len(cnt)
            self.min, self.max = np.full(B, np.inf), np.full(B, -np.inf)
            self.sum, self.count, self.nonfinite = np.zeros(B), np.zeros(B, np.int64), np.zeros(B, np.int64)
        has = cnt > 0
        self.min = np.where(has, np.fmin(self.min, mn), self.min)
        self.max = np.where(has, np.fmax(self.max, mx), self.max)
        self.sum = self.sum + np.where(has, sm, 0.0)
        self.count = self.count + cnt
        self.nonfinite = self.nonfinite + bad


class _SummaryBase:
    def __init__(self, nbins: int = MAX_BINS, per_env: bool = False):
        self.range = HistogramRange(nbins)
        self.per_env = bool(per_env)
        self._m = _Moments()
        self._hist = None       # [B, nbins] int64 (device tensor / NumPy array)
        self._extra = None      # [nbins] int64: counts merged in from summaries of another batch size (pooled mode)
        self._magnitude: Optional[bool] = None

    # ---- range bookkeeping shared by both twins
    def _fit(self, vmin: float, vmax: float, magnitude: bool, width: float = 0.0) -> None:
        if self._magnitude is None:
            self._magnitude = magnitude
        if self.range.lo is None:
            self.range.start(vmin, vmax, magnitude)
            return
        for d in self.range.cover(vmin, vmax, width):
            if self._hist is not None:
                self._hist = HistogramRange.fold(self._hist, d)
            if self._extra is not None:
                self._extra = HistogramRange.fold(self._extra, d)

    @property
    def count(self) -> int:
        return 0 if self._m.count is None else int(self._m.count.sum())

    @property
    def nonfinite(self) -> int:
        return 0 if self._m.nonfinite is None else int(self._m.nonfinite.sum())

    def _host_hist(self) -> np.ndarray:
        raise NotImplementedError

    def histogram(self) -> np.ndarray:
        """Counts on the host: ``[B, nbins]`` with ``per_env``, else pooled ``[nbins]``."""
        h = np.zeros((1, self.range.nbins), np.int64) if self._hist is None else self._host_hist()
        if self.per_env:
            return h
        h = h.sum(axis=0)
        return h if self._extra is None else h + self._to_host(self._extra)

    @staticmethod
    def _to_host(x) -> np.ndarray:
        return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)

    def stats(self) -> Union[Stats, List[Stats]]:
        """``Stats`` over everything seen so far (``per_env``: one per env).  mean = sum / count is exact to rounding, min and
        max are exact, the percentiles are within one bin width (``self.range.width``) wherever the distribution has no empty gap
        at that level (inside a gap every value is a valid quantile)."""
        if self._m.count is None:
            raise RuntimeError("FieldSummary.stats() before the first update()")
        h, m, r = self.histogram(), self._m, self.range
        if self.per_env:
            return [stats_from_histogram(h[b], r.lo, r.width, m.sum[b], m.min[b], m.max[b]) for b in range(h.shape[0])]
        return stats_from_histogram(h, r.lo, r.width, float(np.sum(m.sum)), float(np.min(m.min)), float(np.max(m.max)))

    def merge(self, other: "_SummaryBase") -> "_SummaryBase":
        """Add ``other``'s samples to this summary.  This range is first widened to cover ``other``'s values with bins at least
        as wide as ``other``'s; ``other``'s counts are then assigned by bin centre.  That is exact whenever ``other``'s bins nest
        in this grid (always for magnitudes, whose grids start at 0; for components whenever this ``lo`` is a multiple of
        ``other``'s width); otherwise a count moves by less than one bin width of this summary.
        Moments merge exactly.  ``per_env`` summaries need the same batch size."""
        if other._m.count is None:
            return self
        if other.range.nbins != self.range.nbins:
            raise ValueError("merge: both summaries need the same number of bins")
        if self.per_env and (not other.per_env or (self._m.count is not None and len(other._m.count) != len(self._m.count))):
            raise ValueError("merge: per-env summaries need the same batch size")
        oh = other.histogram() if self.per_env else other.histogram()[None]
        olo, owidth = other.range.lo, other.range.width
        if olo is not None:
            omin, omax = float(np.min(other._m.min)), float(np.max(other._m.max))
            if not hasattr(self, "_device"):
                self._device = getattr(other, "_device", None)
            if self.range.lo is None:
                self.range.lo, self.range.width, self._magnitude = olo, owidth, other._magnitude
            else:
                self._fit(omin, omax, bool(self._magnitude), width=owidth)
            if (olo, owidth) != (self.range.lo, self.range.width):
                centres = olo + (np.arange(self.range.nbins) + 0.5) * owidth
                idx = bin_index(centres, self.range.lo, self.range.width, self.range.nbins)
                moved = np.zeros_like(oh)
                for b in range(oh.shape[0]):
                    np.add.at(moved[b], idx, oh[b])
                oh = moved
            if self.per_env:
                self._hist = self._from_host(oh) if self._hist is None else self._hist + self._from_host(oh)
            else:
                add = self._from_host(oh[0])
                self._extra = add if self._extra is None else self._extra + add
        m, o = self._m, other._m
        if self.per_env or m.count is None or len(m.count) == len(o.count):
            m.add(o.min, o.max, o.sum, o.count, o.nonfinite)
        else:   # pooled summaries of different batch sizes: the other one's moments join env 0
            B = len(m.count)
            pad = lambda v, fill: np.concatenate([[v], np.full(B - 1, fill)])
            m.add(pad(np.min(o.min), np.inf), pad(np.max(o.max), -np.inf), pad(np.sum(o.sum), 0.0),
                  pad(int(np.sum(o.count)), 0).astype(np.int64), pad(int(np.sum(o.nonfinite)), 0).astype(np.int64))
        return self


class HostFieldSummary(_SummaryBase):
    """The NumPy twin of ``FieldSummary``: same range growth, same bin expression, values ``[B, C, ...]`` on the host."""

    def _new_hist(self, B: int):
        return np.zeros((B, self.range.nbins), np.int64)

    def _from_host(self, x):
        return np.asarray(x, np.int64)

    def _host_hist(self) -> np.ndarray:
        return self._hist

    def update(self, field: np.ndarray, channel: Optional[int] = None) -> None:
        f = np.asarray(field, np.float64)
        f = f.reshape(f.shape[0], f.shape[1], -1)
        if channel is None:
            v = np.zeros((f.shape[0], f.shape[2]))
            for c in range(f.shape[1]):
                v = v + f[:, c] * f[:, c]
            v = np.sqrt(v)
        else:
            v = f[:, channel]
        ok = np.isfinite(v)
        cnt = ok.sum(axis=1).astype(np.int64)
        mn = np.array([v[b][ok[b]].min() if cnt[b] else np.nan for b in range(len(v))])
        mx = np.array([v[b][ok[b]].max() if cnt[b] else np.nan for b in range(len(v))])
        sm = np.array([v[b][ok[b]].sum() for b in range(len(v))])
        self._m.add(mn, mx, sm, cnt, (~ok).sum(axis=1).astype(np.int64))
        if not cnt.any():
            return
        if self._hist is None:
            self._hist = self._new_hist(len(v))
        self._fit(float(np.nanmin(mn)), float(np.nanmax(mx)), channel is None)
        r = self.range
        for b in range(len(v)):
            self._hist[b] += np.bincount(bin_index(v[b][ok[b]], r.lo, r.width, r.nbins), minlength=r.nbins)


class FieldSummary(_SummaryBase):
    """Running summary of a device field over the samples of a rollout.

    ``update(field, channel=None)``: ``field [B, C, ...]`` contiguous on the GPU (float32 -> ``libfluidgym_hip.so``, float64 ->
    the fp64 library); ``channel=None`` summarises the Euclidean magnitude over ``C``.  One update is the moments launch, ONE
    host read of ``[B, 5]`` numbers (which synchronises: this is off the step path), a range growth if the sample needs it, and the
    histogram launch.  ``fused=True`` reads the field once instead: moments and a histogram over the CURRENT range go in one
    launch into a scratch histogram that is added when the sample turned out to fit, and redone after a growth when not
    (measured in profiles/field_stats_cost.py; the default is the cheaper form at the headline shape).
    """

    def __init__(self, nbins: int = MAX_BINS, per_env: bool = False, fused: bool = False):
        super().__init__(nbins, per_env)
        self.fused = bool(fused)
        self._bufs = None

    def _new_hist(self, B: int):
        return torch.zeros(B, self.range.nbins, dtype=torch.int64, device=self._device)

    def _from_host(self, x):
        return torch.as_tensor(np.asarray(x, np.int64), device=self._device)

    def _host_hist(self) -> np.ndarray:
        return self._hist.cpu().numpy()

    def _launch(self, lib, field, B, C, n, channel, moments: bool, hist) -> None:
        work, mom, cnt = self._bufs
        null = ctypes.c_void_p(None)
        r = self.range
        L.check(lib.fg_field_summary(
            ctypes.c_void_p(field.data_ptr()), B, C, n, channel,
            ctypes.c_void_p(work.data_ptr()) if moments else null, ctypes.c_void_p(mom.data_ptr()) if moments else null,
            ctypes.c_void_p(cnt.data_ptr()) if moments else null,
            float(r.lo) if hist is not None else 0.0, float(r.width) if hist is not None else 1.0, r.nbins,
            ctypes.c_void_p(hist.data_ptr()) if hist is not None else null,
            ctypes.c_void_p(torch.cuda.current_stream(field.device).cuda_stream)), lib=lib)

    def update(self, field: torch.Tensor, channel: Optional[int] = None) -> None:
        if not field.is_cuda:
            raise ValueError("FieldSummary.update: the field must live on the GPU (HostFieldSummary takes host arrays)")
        if field.dim() < 2:
            raise ValueError("FieldSummary.update: field must be [B, C, ...]")
        if field.dtype not in (torch.float32, torch.float64):
            raise TypeError(f"FieldSummary.update: float32 or float64 fields, got {field.dtype}")
        field = field.contiguous()
        B, C = int(field.shape[0]), int(field.shape[1])
        n = int(field[0, 0].numel())
        if channel is not None and not 0 <= int(channel) < C:
            raise ValueError(f"FieldSummary.update: channel {channel} out of range for {C} channels")
        lib = L.load_f64() if field.dtype == torch.float64 else L.load()
        dev = field.device
        if self._bufs is None or self._bufs[1].shape[0] != B or self._bufs[1].device != dev:
            if self._hist is not None and (self._hist.shape[0] != B or self._hist.device != dev):
                raise ValueError("FieldSummary.update: batch size or device changed between updates")
            self._device = dev
            self._bufs = (torch.empty(B * L.FG_FIELD_SUMMARY_WORK_BYTES, dtype=torch.uint8, device=dev),
                          torch.empty(B, 3, dtype=torch.float64, device=dev), torch.empty(B, 2, dtype=torch.int64, device=dev))
        ch = -1 if channel is None else int(channel)
        with torch.cuda.device(dev):
            scratch = None
            if self.fused and self.range.lo is not None:
                scratch = torch.zeros(B, self.range.nbins, dtype=torch.int64, device=dev)
                self._launch(lib, field, B, C, n, ch, True, scratch)
            else:
                self._launch(lib, field, B, C, n, ch, True, None)
            _, mom, cnt = self._bufs
            host = torch.cat([mom, cnt.to(torch.float64)], dim=1).cpu().numpy()     # the one host read of the sample
            counts = host[:, 3:].astype(np.int64)
            self._m.add(host[:, 0], host[:, 1], host[:, 2], counts[:, 0], counts[:, 1])
            if not counts[:, 0].any():
                return
            if self._hist is None:
                self._hist = self._new_hist(B)
            before = (self.range.lo, self.range.width)
            self._fit(float(np.nanmin(host[:, 0])), float(np.nanmax(host[:, 1])), channel is None)
            if scratch is not None and before == (self.range.lo, self.range.width):
                self._hist += scratch
            else:
                self._launch(lib, field, B, C, n, ch, False, self._hist)
