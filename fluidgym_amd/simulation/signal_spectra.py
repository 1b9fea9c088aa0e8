"""Online Welch power and cross spectra of per-env scalar signals: at which frequency a drag, a lift, a probe value lives, and how
coherent two of them are.

A recorder takes one sample -- ``S`` numbers per env -- per call and keeps, per env, a ring of the last ``L = segment`` samples and
a counter ``fill`` of the samples since the env last (re)started.  Whenever ``fill >= L`` and ``(fill - L) % hop == 0`` with
``hop = L - noverlap`` a segment is due: the ring in time order is detrended per signal (``"none"``, ``"constant"``: the mean,
``"linear"``: the least-squares line; sums in fp64), multiplied by the window, rounded to the dtype of the signals and transformed;
``|X_s|^2`` is added to ``power [B, S, L/2+1]``, ``conj(X_a) X_b`` of the listed pairs to ``cross [B, n_pairs, L/2+1]`` (SciPy's
``csd`` convention), ``1`` to ``segments [B]``, and ``last [B, S, L/2+1]`` is overwritten.  ``restart(envs)`` zeroes ``fill`` of the chosen
envs: their open segment is dropped, so that no segment straddles an episode boundary, and the sums stay.  The envs of a batch are
therefore out of phase with each other, and the schedule is kept per env, on the device.

The accessors scale the sums to the one-sided ``density`` estimate averaged over the segments: ``psd`` and ``csd`` are
``scipy.signal.welch`` / ``scipy.signal.csd`` with ``average="mean"`` of every uninterrupted piece of the series, weighted by the
pieces' segment counts.  An env without a segment gives NaN.

``SignalSpectra`` accumulates on the GPU: one sample of a batch is one launch of ``fg_signal_spectra``
(``csrc/fg_signalspectra.hip``) that reads up to 8 source tensors in place and returns nothing to the host.
``HostSignalSpectra`` is its NumPy fp64 twin (the reference of the tests): same schedule, the ring rounded to the dtype of the
signals; both share ``SignalSpectraRecord``: the spec, the accessors, ``merge`` / ``pooled`` and the files.
"""
from __future__ import annotations

import ctypes
import json
import os
from typing import Optional, Sequence, Tuple, Union

import numpy as np
import torch

from .. import _lib as L
from . import plane_fields as F

MAX_SOURCES, MAX_SIGNALS, MAX_PAIRS = 8, 64, 64
MIN_SEGMENT = 16
LDS_LIMIT = 160 * 1024
DETRENDS = ("none", "constant", "linear")
FILE_RECORD, FILE_META = "signal_spectra.npz", "signal_spectra.json"


def max_segment(dtype) -> int:
    """The longest segment ``fg_signal_spectra`` takes for signals of ``dtype``: twiddles and the three work buffers of one wave,
    four arrays of ``segment`` complex numbers, fit in 160 KB of LDS -- 4096 for float32, 2048 for float64."""
    itemsize = 8 if dtype in (torch.float64, np.float64, np.dtype(np.float64)) else 4
    n = MIN_SEGMENT
    while 4 * (2 * n) * 2 * itemsize <= LDS_LIMIT:
        n *= 2
    return n


def check_extents(segment: int, dtype=None, what: str = "SignalSpectra") -> None:
    """The extents rule of ``fg_signal_spectra`` restated: a power of two, at least 16, at most ``max_segment(dtype)`` (``dtype`` None:
    the rule of float32, the wider one)."""
    segment = int(segment)
    if segment < MIN_SEGMENT or segment & (segment - 1):
        raise ValueError(f"{what}: segment must be a power of two, at least {MIN_SEGMENT}, got {segment}")
    top = max_segment(torch.float32 if dtype is None else dtype)
    if segment > top:
        raise ValueError(f"{what}: segment = {segment} does not fit in 160 KB of LDS for {dtype or 'float32'} signals (at most {top})")


def make_window(window, segment: int) -> Tuple[Optional[str], np.ndarray]:
    """``(name or None, w [L] in fp64)``: a ``scipy.signal.get_window`` name (the periodic form ``welch`` uses) or an array."""
    if isinstance(window, (str, tuple)):
        from scipy.signal import get_window

        return (window if isinstance(window, str) else None), np.asarray(get_window(window, segment), np.float64)
    w = np.array(window, np.float64)
    if w.shape != (segment,):
        raise ValueError(f"window must be a scipy.signal.get_window name or an array [{segment}], got shape {w.shape}")
    if not np.all(np.isfinite(w)) or not np.any(w != 0.0):
        raise ValueError("window must be finite and not all zero")
    return None, w


def segment_spectra(seg: np.ndarray, window: np.ndarray, detrend: int, dtype) -> np.ndarray:
    """The spectra ``[..., S, L/2+1]`` (complex, unnormalised) of segments ``[..., S, L]`` as ``fg_signal_spectra`` takes them, in
    fp64 but for the one rounding to ``dtype`` before the transform; a signal with a non-finite sample is NaN."""
    v = np.asarray(seg, np.float64)
    n = v.shape[-1]
    tc = np.arange(n) - 0.5 * (n - 1)
    with np.errstate(all="ignore"):
        mean = v.sum(axis=-1, keepdims=True) / n if detrend else 0.0
        slope = (v * tc).sum(axis=-1, keepdims=True) / (n * (float(n) * n - 1.0) / 12.0) if detrend == 2 else 0.0
        y = ((v - (mean + slope * tc)) * window).astype(dtype).astype(np.float64)
        bad = ~np.isfinite(v).all(axis=-1, keepdims=True)
        X = np.fft.rfft(np.where(bad, 0.0, y), axis=-1)
    return np.where(bad, complex(np.nan, np.nan), X)


class SignalSpectraRecord:
    """Spec, accessors, merging and files of a record; the two accumulators below say where the arrays live.

    ``names``: the signals; ``segment``: ``L``; ``noverlap`` (default ``L // 2``); ``window``: a ``scipy.signal.get_window`` name or an
    array ``[L]``; ``detrend``: ``"none"``, ``"constant"`` or ``"linear"``; ``pairs``: ``(a, b)`` by name, the cross spectra kept;
    ``dt``: the sample interval."""

    def __init__(self, names: Sequence[str], segment: int = 256, noverlap: Optional[int] = None, window="hann",
                 detrend: str = "constant", pairs: Sequence[Tuple[str, str]] = (), dt: float = 1.0):
        names = tuple(str(n) for n in names)
        if not names or len(set(names)) != len(names) or len(names) > MAX_SIGNALS:
            raise ValueError(f"names must be 1..{MAX_SIGNALS} distinct signal names, got {names}")
        check_extents(segment, None, type(self).__name__)
        self.names, self.segment = names, int(segment)
        self.noverlap = self.segment // 2 if noverlap is None else int(noverlap)
        if not 0 <= self.noverlap < self.segment:
            raise ValueError(f"noverlap must lie in [0, segment = {self.segment}), got {noverlap}")
        if detrend not in DETRENDS:
            raise ValueError(f"detrend must be one of {DETRENDS}, got {detrend!r}")
        self.detrend = detrend
        self.window_name, self.window = make_window(window, self.segment)
        self.pairs = tuple((str(a), str(b)) for a, b in pairs)
        if len(self.pairs) > MAX_PAIRS or len(set(self.pairs)) != len(self.pairs):
            raise ValueError(f"pairs must be at most {MAX_PAIRS} distinct (a, b), got {self.pairs}")
        for a, b in self.pairs:
            if a not in names or b not in names:
                raise ValueError(f"pair ({a!r}, {b!r}) names a signal that is not recorded: {names}")
        if not float(dt) > 0.0:
            raise ValueError(f"dt, the sample interval, must be positive, got {dt}")
        self.dt = float(dt)
        self.S, self.hop, self.bins = len(names), self.segment - self.noverlap, self.segment // 2 + 1

    def spec(self) -> dict:
        return {"names": list(self.names), "segment": self.segment, "noverlap": self.noverlap, "window": self.window_name,
                "detrend": self.detrend, "pairs": [list(p) for p in self.pairs], "dt": self.dt}

    def _same_spec(self, other: "SignalSpectraRecord") -> bool:
        mine, theirs = self.spec(), other.spec()
        mine.pop("window"), theirs.pop("window")
        return mine == theirs and np.array_equal(self.window, other.window)

    # ---- where the arrays live: (power [B, S, H], cross [B, P, H, 2], last [B, S, H], segments [B]) on the host
    _arrays = None

    def _state(self):
        if self._arrays is None:
            raise RuntimeError("no sample recorded yet")
        return self._arrays

    def _set_state(self, power, cross, last, segments) -> None:
        self._arrays = (np.ascontiguousarray(power, np.float64), np.ascontiguousarray(cross, np.float64),
                        np.ascontiguousarray(last, np.float64), np.ascontiguousarray(segments, np.int64))

    def _unset(self) -> bool:
        return self._arrays is None

    def _like(self, power, cross, last, segments) -> "HostSignalSpectra":
        r = HostSignalSpectra(self.names, self.segment, self.noverlap, self.window, self.detrend, self.pairs, self.dt)
        r.window_name = self.window_name
        r._set_state(power, cross, last, segments)
        return r

    def record(self) -> "HostSignalSpectra":
        """A host copy of the sums (not of the rings: it serves the accessors, ``merge``, ``pooled`` and ``save``)."""
        return self._like(*(np.array(a) for a in self._state()))

    @property
    def segments(self) -> np.ndarray:
        """Segments behind every env's sums, ``[B]``."""
        return self._state()[3]

    # ---- accessors, per env
    def _sig(self, name: Union[int, str]) -> int:
        if isinstance(name, str):
            if name not in self.names:
                raise KeyError(f"no signal {name!r}: the record holds {self.names}")
            return self.names.index(name)
        return int(name)

    def frequencies(self) -> np.ndarray:
        """``[L/2+1]``, in cycles per unit of ``dt``."""
        return np.fft.rfftfreq(self.segment, self.dt)

    def _scale(self) -> np.ndarray:
        """Sum over segments -> one-sided density per segment sum: ``dt / sum(w^2)``, doubled but for DC and Nyquist."""
        s = np.full(self.bins, 2.0 * self.dt / float((self.window * self.window).sum()))
        s[0] *= 0.5
        s[-1] *= 0.5
        return s

    def _mean(self, total: np.ndarray) -> np.ndarray:
        n = self.segments.astype(np.float64)
        n = np.where(n > 0, n, np.nan).reshape((-1,) + (1,) * (total.ndim - 1))
        return total * self._scale() / n

    def psd(self, name) -> np.ndarray:
        """The power spectral density ``[B, L/2+1]``: ``scipy.signal.welch(..., scaling="density", average="mean")``."""
        return self._mean(self._state()[0][:, self._sig(name)])

    def csd(self, a, b) -> np.ndarray:
        """The cross spectral density ``[B, L/2+1]`` (complex, ``conj(X_a) X_b``: ``scipy.signal.csd``) of a listed pair; a pair listed
        the other way round is conjugated, a signal with itself is its ``psd``."""
        a, b = self.names[self._sig(a)], self.names[self._sig(b)]
        cross = self._state()[1]
        if (a, b) in self.pairs:
            c = cross[:, self.pairs.index((a, b))]
            return self._mean(c[..., 0]) + 1j * self._mean(c[..., 1])      # (scaled part by part, as psd is)
        if (b, a) in self.pairs:
            c = cross[:, self.pairs.index((b, a))]
            return self._mean(c[..., 0]) - 1j * self._mean(c[..., 1])
        if a == b:
            return self.psd(a).astype(np.complex128)
        raise KeyError(f"the pair ({a!r}, {b!r}) is not recorded: list it in pairs (the record holds {self.pairs})")

    def coherence(self, a, b) -> np.ndarray:
        """Magnitude-squared coherence ``|P_ab|^2 / (P_aa P_bb)``, ``[B, L/2+1]``."""
        c = self.csd(a, b)
        with np.errstate(all="ignore"):
            return (c.real * c.real + c.imag * c.imag) / (self.psd(a) * self.psd(b))

    def phase(self, a, b) -> np.ndarray:
        """The phase of ``csd(a, b)`` in radians: positive where ``b`` leads ``a``."""
        return np.angle(self.csd(a, b))

    def latest(self, name) -> np.ndarray:
        """The density of the last processed segment alone, ``[B, L/2+1]`` (NaN before an env's first segment)."""
        last = self._state()[2][:, self._sig(name)] * self._scale()
        return np.where((self.segments > 0)[:, None], last, np.nan)

    def peak_frequency(self, name, band: Optional[Tuple[float, float]] = None) -> np.ndarray:
        """Per env the frequency of the largest bin of ``psd(name)`` inside ``band = (f_lo, f_hi)`` (default: all but DC), refined by the
        parabola through the logarithms of the bin and its two neighbours; ``[B]``."""
        P, f = self.psd(name), self.frequencies()
        lo, hi = (f[1], f[-1]) if band is None else (float(band[0]), float(band[1]))
        inside = (f >= lo) & (f <= hi)
        if not inside.any():
            raise ValueError(f"band {band} holds no bin of {f[0]} .. {f[-1]}")
        out = np.full(P.shape[0], np.nan)
        for e in range(P.shape[0]):
            if not np.isfinite(P[e][inside]).all():
                continue
            k = int(np.argmax(np.where(inside, P[e], -np.inf)))
            shift = 0.0
            if 0 < k < self.bins - 1 and min(P[e, k - 1], P[e, k], P[e, k + 1]) > 0.0:
                la, lb, lc = np.log(P[e, k - 1:k + 2])
                curve = la - 2.0 * lb + lc
                shift = 0.5 * (la - lc) / curve if curve < 0.0 else 0.0
            out[e] = (k + shift) * (f[1] - f[0])
        return out

    def strouhal(self, name, length: float, velocity: float, band: Optional[Tuple[float, float]] = None) -> np.ndarray:
        """``peak_frequency(name) * length / velocity`` per env."""
        return self.peak_frequency(name, band) * float(length) / float(velocity)

    # ---- merging
    def merge(self, other: "SignalSpectraRecord") -> "SignalSpectraRecord":
        """Add ``other``'s sums and segment counts (same spec and batch size) to this record, env by env; ``last`` becomes
        ``other``'s where ``other`` has a segment."""
        if not self._same_spec(other):
            raise ValueError("merge: both records need the same names, segment, noverlap, window, detrend, pairs and dt")
        theirs = other._state()
        if self._unset():
            raise RuntimeError("merge: this record has no sample yet (merge into other.record() instead)")
        mine = self._state()
        if mine[0].shape != theirs[0].shape:
            raise ValueError(f"merge: batch sizes differ, {mine[0].shape[0]} and {theirs[0].shape[0]}")
        last = np.where((theirs[3] > 0)[:, None, None], theirs[2], mine[2])
        self._set_state(mine[0] + theirs[0], mine[1] + theirs[1], last, mine[3] + theirs[3])
        return self

    def pooled(self) -> "HostSignalSpectra":
        """The envs of the batch summed into one ensemble record (``B = 1``) on the host; ``last`` is that of the last env with a
        segment."""
        power, cross, last, seg = self._state()
        have = np.nonzero(seg > 0)[0]
        keep = last[have[-1]:have[-1] + 1] if have.size else last[:1] * 0.0
        return self._like(power.sum(axis=0, keepdims=True), cross.sum(axis=0, keepdims=True), keep, seg.sum(keepdims=True))

    # ---- files
    def save(self, path) -> None:
        """``<path>.npz`` (the sums, the segment counts, the window) and ``<path>.json`` (the spec); ``path`` without a suffix."""
        base = os.path.splitext(str(path))[0]
        os.makedirs(os.path.dirname(os.path.abspath(base)), exist_ok=True)
        power, cross, last, seg = self._state()
        np.savez_compressed(base + ".npz", power=power, cross=cross, last=last, segments=seg, window=self.window)
        with open(base + ".json", "w") as f:
            json.dump(self.spec(), f, indent=1)

    @staticmethod
    def load(path) -> "HostSignalSpectra":
        base = os.path.splitext(str(path))[0]
        with open(base + ".json") as f:
            meta = json.load(f)
        with np.load(base + ".npz") as z:
            r = HostSignalSpectra(meta["names"], meta["segment"], meta["noverlap"], z["window"], meta["detrend"],
                                  [tuple(p) for p in meta["pairs"]], meta["dt"])
            r.window_name = meta["window"]
            r._set_state(z["power"], z["cross"], z["last"], z["segments"])
        return r

    # ---- what both accumulators check of a sample
    def _widths(self, shapes, what: str) -> Tuple[int, list]:
        if not 1 <= len(shapes) <= MAX_SOURCES:
            raise ValueError(f"{what}: 1..{MAX_SOURCES} sources per sample, got {len(shapes)}")
        B = int(shapes[0][0]) if len(shapes[0]) else 0
        widths = []
        for s in shapes:
            if len(s) not in (1, 2) or int(s[0]) != B or B < 1 or (len(s) == 2 and int(s[1]) < 1):
                raise ValueError(f"{what}: every source must be [B] or [B, n] with one B >= 1, got {[tuple(t) for t in shapes]}")
            widths.append(1 if len(s) == 1 else int(s[1]))
        if sum(widths) != self.S:
            raise ValueError(f"{what}: the sources hold {sum(widths)} signals, the record has {self.S} names")
        return B, widths

    def _pair_index(self) -> np.ndarray:
        return np.array([[self.names.index(a), self.names.index(b)] for a, b in self.pairs], np.int32).reshape(-1, 2)


class HostSignalSpectra(SignalSpectraRecord):
    """The NumPy fp64 twin of ``SignalSpectra``: same schedule and arithmetic, arrays on the host; the ring is rounded to the dtype of
    the signals it was fed (float32 or float64, taken from the first sample), as on the device."""

    _ring = _fill = None

    def update(self, *sources) -> None:
        what = "HostSignalSpectra.update"
        arrs = [np.asarray(s) for s in sources]
        B, _ = self._widths([a.shape for a in arrs], what)
        if self._ring is None:
            dtype = arrs[0].dtype if arrs[0].dtype in (np.float32, np.float64) else np.dtype(np.float64)
            check_extents(self.segment, dtype, what)
            self._ring, self._fill = np.zeros((B, self.S, self.segment), dtype), np.zeros(B, np.int64)
            if self._arrays is None:
                self._set_state(np.zeros((B, self.S, self.bins)), np.zeros((B, len(self.pairs), self.bins, 2)),
                                np.zeros((B, self.S, self.bins)), np.zeros(B, np.int64))
        if self._ring.shape[0] != B or self._arrays[0].shape[0] != B:
            raise ValueError(f"{what}: batch size changed between updates")
        sample = np.concatenate([a.reshape(B, -1) for a in arrs], axis=1)
        n = self.segment
        self._ring[np.arange(B), :, self._fill % n] = sample.astype(self._ring.dtype)
        self._fill += 1
        due = np.nonzero((self._fill >= n) & ((self._fill - n) % self.hop == 0))[0]
        if not due.size:
            return
        order = (self._fill[due, None] + np.arange(n)[None]) % n                   # the ring in time order, per due env
        seg = np.take_along_axis(self._ring[due], order[:, None, :], axis=2)
        X = segment_spectra(seg, self.window, DETRENDS.index(self.detrend), self._ring.dtype)
        power, cross, last, segments = self._arrays
        p = X.real * X.real + X.imag * X.imag
        power[due] += p
        last[due] = p
        for j, (a, b) in enumerate(self._pair_index()):
            ar, ai, br, bi = X[:, a].real, X[:, a].imag, X[:, b].real, X[:, b].imag
            cross[due, j, :, 0] += ar * br + ai * bi               # conj(X_a) X_b, product by product as the kernel takes it
            cross[due, j, :, 1] += ar * bi - ai * br
        segments[due] += 1

    def restart(self, envs=None) -> None:
        """Drop the open segment of ``envs`` (default: of every env); the sums stay."""
        if self._fill is not None:
            self._fill[slice(None) if envs is None else np.asarray(envs)] = 0


class SignalSpectra(SignalSpectraRecord):
    """The GPU accumulator.  ``update(*sources)`` takes up to 8 GPU tensors ``[B]`` or ``[B, n_i]`` of one dtype (float32 ->
    ``libfluidgym_hip.so``, float64 -> the fp64 library), reads them in place and runs one launch on the current stream; nothing
    comes back to the host until an accessor is called."""

    # _dev: power, cross, last, segments (the record), then ring, fill, window
    _dev = None
    _shape = None

    def _state(self):
        if self._dev is None:
            raise RuntimeError("no sample recorded yet")
        return tuple(t.cpu().numpy() for t in self._dev[:4])

    def _set_state(self, power, cross, last, segments) -> None:
        if self._dev is None:
            raise RuntimeError("SignalSpectra takes a state only after its first update (merge into a record() instead)")
        for t, v in zip(self._dev[:4], (power, cross, last, segments)):
            t.copy_(torch.as_tensor(np.ascontiguousarray(v)).reshape(t.shape).to(t.dtype))

    def _unset(self) -> bool:
        return self._dev is None

    def update(self, *sources) -> None:
        what = "SignalSpectra.update"
        if sources:
            F.check_device_fields(sources, what, "HostSignalSpectra")
        B, widths = self._widths([tuple(t.shape) for t in sources], what)
        first = sources[0]
        dev, dtype = first.device, first.dtype
        if self._dev is None:
            check_extents(self.segment, dtype, what)
            z = dict(dtype=torch.float64, device=dev)
            self._shape = (B, dev, dtype)
            self._dev = (torch.zeros(B, self.S, self.bins, **z), torch.zeros(B, len(self.pairs), self.bins, 2, **z),
                         torch.zeros(B, self.S, self.bins, **z), torch.zeros(B, dtype=torch.int64, device=dev),
                         torch.zeros(B, self.S, self.segment, dtype=dtype, device=dev), torch.zeros(B, dtype=torch.int64, device=dev),
                         torch.as_tensor(self.window, dtype=torch.float64).to(dev))
            pairs = self._pair_index()
            self._pairs_c = (ctypes.c_int32 * max(pairs.size, 1))(*pairs.reshape(-1).tolist())
        elif self._shape != (B, dev, dtype):
            raise ValueError(f"{what}: batch size, dtype or device changed between updates")
        # read in place: a column stride of one element, any batch stride at least the width
        held = [t if (t.dim() == 1 or t.shape[1] == 1 or t.stride(1) == 1) and t.stride(0) >= w else t.contiguous()
                for t, w in zip(sources, widths)]
        n = len(held)
        ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in held])
        strides = (ctypes.c_int64 * n)(*[int(t.stride(0)) if B > 1 else w for t, w in zip(held, widths)])
        wid = (ctypes.c_int32 * n)(*widths)
        power, cross, last, segments, ring, fill, window = self._dev
        lib = F.library(dtype)
        with torch.cuda.device(dev):
            L.check(lib.fg_signal_spectra(ptrs, strides, wid, n, B, self.segment, self.noverlap, DETRENDS.index(self.detrend), F.ptr(window),
                                          self._pairs_c, len(self.pairs), F.ptr(ring), F.ptr(fill), F.ptr(power),
                                          F.ptr(cross) if self.pairs else None, F.ptr(segments), F.ptr(last), F.stream_ptr(dev)), lib=lib)

    def restart(self, envs=None) -> None:
        """Drop the open segment of ``envs`` (default: of every env) with one index op on the device; the sums stay."""
        if self._dev is None:
            return
        fill = self._dev[5]
        if envs is None:
            fill.zero_()
        else:
            fill.index_fill_(0, torch.as_tensor(np.asarray(envs).reshape(-1), dtype=torch.int64, device=fill.device), 0)
