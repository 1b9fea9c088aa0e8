"""Online per-cell flow statistics of the multi-block domains (cylinder, airfoil): time-averaged velocity and pressure, Reynolds
stresses and ``p'^2`` per cell, in 3-D averaged over the periodic span as well.

The reference's tools for this are ``WelfordOnlineParallel_Torch`` and ``CovarianceOnlineParallel_Torch``
(``pict/data/online_statistics.py:31-266``) applied per block with ``dims=[0]`` in 2-D and ``dims=[0, 2]`` in 3-D: per sample, block
and statistic a ``torch.mean``, a full-field difference and a ``torch.sum``.  Here one sample of a batch of ``B`` envs is one launch of
``fg_mb_cell_moments`` (``csrc/fg_cellstats.hip``) over the flat fields ``velocity [B, d, N]``, ``pressure [B, N]`` of a
``MultiBlockDomain``; nothing comes back to the host until an accessor is called.

A *column* is ``(block, y, x)``: the ``nz`` cells along the span of a 3-D block with ``span_average=True``, one cell otherwise (then
every cell is a column and a 3-D block's arrays are ``[B, nz, ny, nx]``).  A record holds the number of merged samples and, per env
and column, the ``K = d + 1`` means of ``u, v(, w), p`` and the ``K (K + 1) / 2`` sums of ``d_i d_j`` (``i <= j``, ``d`` = deviation
from the mean) as ``mean [B, K, NC]`` and ``central [B, P, NC]`` with the columns in domain order (block after block, ``x`` fastest).
A column has seen ``n = samples * nz`` cells.  Records merge by the order-2 rule of ``plane_stats.merge_moments`` (parallel Welford /
Schubert-Gertz, ``delta = mean_B - mean_A``).

``CellMoments`` accumulates on the GPU, ``HostCellMoments`` is its NumPy fp64 twin.  Both share the accessors, ``merge`` / ``pooled``
and the files.

Files.  ``save(directory)`` writes env ``b`` into ``directory/env_%04d``, ``save(directory, pooled=True)`` the ensemble of all envs
into ``directory`` itself.  Per directory and block ``i``, in the layouts and with the key names of the reference's ``save`` methods
(arrays ``[C, ny, nx]``, without span averaging in 3-D ``[C, nz, ny, nx]``: what its classes produce with ``squeeze_dims=True``):

    block{i}_vel_stats.npz       n, mean [d, ...], sum_squares [d, ...]        WelfordOnlineParallel_Torch of the velocity
    block{i}_p_stats.npz         n, mean [1, ...], sum_squares [1, ...]        ... of the pressure
    block{i}_vel_cov_{ab}.npz    n, mean_x [1, ...], mean_y [1, ...], C        CovarianceOnlineParallel_Torch of the components a, b
                                                                               (``uv``; in 3-D also ``uw``, ``vw``)

and ``cell_moments.npz`` with the whole state of that env (``load`` reads this one: the pressure-velocity sums are in no reference
file); ``directory/cell_moments.json`` names the blocks, the options and the directories.
"""
from __future__ import annotations

import ctypes
import json
import os
from typing import List, Sequence, Tuple, Union

import numpy as np
import torch

from .. import _lib as L
from . import plane_fields as F
from .plane_stats import merge_moments

MAX_BLOCKS = 8                          # CM_MAX_BLOCKS of csrc/fg_cellstats.hip
FILE_STATE, FILE_META = "cell_moments.npz", "cell_moments.json"


def sample_cell_moments(values: np.ndarray, table: np.ndarray):
    """One sample on the host: ``values [K, B, N]`` and the block table -> ``mean [B, K, NC]``, ``central [B, P, NC]`` by two fp64
    passes.  A column with a non-finite cell in any channel is NaN in every channel, as on the device."""
    v = np.asarray(values, np.float64)
    K, B = v.shape[:2]
    pairs = [(i, j) for i in range(K) for j in range(i, K)]
    NC = int(table[:, 1].sum())
    mean, cen = np.empty((B, K, NC)), np.empty((B, len(pairs), NC))
    with np.errstate(all="ignore"):
        for off, layer, nz, col in table:
            cells = v[:, :, off:off + nz * layer].reshape(K, B, nz, layer)
            m = np.zeros((K, B, layer))
            for z in range(nz):
                m = m + cells[:, :, z]
            m = m / float(nz)
            m = np.where(np.isfinite(m).all(axis=0, keepdims=True), m, np.nan)
            d = cells - m[:, :, None]
            mean[:, :, col:col + layer] = np.moveaxis(m, 0, 1)
            for q, (i, j) in enumerate(pairs):
                c = np.zeros((B, layer))
                for z in range(nz):
                    c = c + d[i, :, z] * d[j, :, z]
                cen[:, q, col:col + layer] = c
    return mean, cen


class CellRecord:
    """Accessors, merging and files of a record ``samples``, ``mean [B, K, NC]``, ``central [B, P, NC]``; the two accumulators below
    say where the arrays live.  ``blocks``: ``(size, cell_offset)`` per block of a prepared ``MultiBlockDomain``, ``size`` =
    ``(nx, ny[, nz])``."""

    def __init__(self, blocks: Sequence[Tuple[Sequence[int], int]], dims: int, span_average: bool = True):
        if int(dims) not in (2, 3):
            raise ValueError(f"dims must be 2 or 3, got {dims}")
        blocks = [(tuple(int(s) for s in size), int(off)) for size, off in blocks]
        if not 1 <= len(blocks) <= MAX_BLOCKS:
            raise ValueError(f"1 to {MAX_BLOCKS} blocks, got {len(blocks)}")
        if any(len(size) != dims or min(size) < 1 or off < 0 for size, off in blocks):
            raise ValueError(f"blocks must be ((nx, ny[, nz]), cell_offset) of a prepared {dims}-D domain, got {blocks}")
        self.blocks, self.dims, self.span_average = blocks, int(dims), bool(span_average)
        self.channels = ("u", "v") + (("w",) if self.dims == 3 else ()) + ("p",)
        self.K = len(self.channels)
        self.pairs = [(i, j) for i in range(self.K) for j in range(i, self.K)]
        self.P = len(self.pairs)
        rows, self.shapes, col = [], [], 0
        for size, off in blocks:
            cells = int(np.prod(size))
            nz = size[2] if self.dims == 3 and self.span_average else 1
            rows.append((off, cells // nz, nz, col))                       # cell_offset, layer_cells, nz, column_offset
            self.shapes.append(tuple(reversed(size[:2] if self.span_average else size)))
            col += cells // nz
        self.table = np.asarray(rows, np.int64)
        self.NC = col
        self.min_cells = int(max(r[0] + r[1] * r[2] for r in rows))
        self.column_n = np.concatenate([np.full(r[1], float(r[2])) for r in rows])      # cells per column and sample, [NC]
        self.samples = 0

    # ---- where the arrays live: overridden by CellMoments
    _mean = _central = None
    surface = None      # the WallMoments recorded beside it (start_field_statistics(surface=True)), else None

    def _state(self):
        if self._mean is None:
            raise RuntimeError("no sample recorded yet")
        return self._mean, self._central

    def _set_state(self, mean, central) -> None:
        self._mean, self._central = (np.ascontiguousarray(v, np.float64) for v in (mean, central))

    def _unset(self) -> bool:
        return self._mean is None

    def _like(self, samples: int, mean, central) -> "HostCellMoments":
        r = HostCellMoments(self.blocks, self.dims, self.span_average)
        r._set_state(mean, central)
        r.samples = int(samples)
        return r

    def record(self) -> "HostCellMoments":
        """A host copy of the current state."""
        return self._like(self.samples, *(np.array(v) for v in self._state()))

    # ---- accessors: flat("mean", ch) etc. are [B, NC] in domain order, the named forms [B, (nz,) ny, nx] of one block
    def _ch(self, ch: Union[int, str]) -> int:
        return self.channels.index(ch) if isinstance(ch, str) else int(ch)

    def _pair(self, i, j) -> int:
        i, j = sorted((self._ch(i), self._ch(j)))
        return self.pairs.index((i, j))

    def flat(self, what: str, *args) -> np.ndarray:
        """``flat("n")``, ``flat("mean", ch)``, ``flat("covariance", i, j)``, ``flat("variance", ch)``, ``flat("tke")``: ``[B, NC]``."""
        mean, cen = self._state()
        n = self.samples * self.column_n
        if what == "n":
            return np.broadcast_to(n, mean.shape[::2]).copy()
        if what == "mean":
            return np.array(mean[:, self._ch(args[0])])
        if what == "covariance":
            return cen[:, self._pair(*args)] / n
        if what == "variance":
            return cen[:, self._pair(args[0], args[0])] / n
        if what == "tke":
            return 0.5 * sum(cen[:, self._pair(c, c)] for c in range(self.K - 1)) / n
        raise KeyError(f"flat: unknown statistic {what!r}")

    def _block(self, flat: np.ndarray, block: int) -> np.ndarray:
        _, layer, _, col = self.table[block]
        return flat[:, col:col + layer].reshape((flat.shape[0],) + self.shapes[block])

    def n(self, block: int) -> float:
        """Cells every column of ``block`` has seen: ``samples * nz`` (``nz`` = 1 without span averaging)."""
        return float(self.samples * self.table[block][2])

    def mean(self, ch, block: int) -> np.ndarray:
        return self._block(self.flat("mean", ch), block)

    def covariance(self, i, j, block: int) -> np.ndarray:
        return self._block(self.flat("covariance", i, j), block)

    def variance(self, ch, block: int) -> np.ndarray:
        return self._block(self.flat("variance", ch), block)

    def tke(self, block: int) -> np.ndarray:
        return self._block(self.flat("tke"), block)

    def at_cells(self, ch, index) -> Tuple[np.ndarray, np.ndarray]:
        """Mean and variance of a channel at the flat column indices ``index`` (e.g. the wall-adjacent cells of a surface, for its
        mean and r.m.s. pressure): two ``[B, len(index)]`` arrays."""
        index = np.asarray(index.cpu() if isinstance(index, torch.Tensor) else index, np.int64).reshape(-1)
        if len(index) and (index.min() < 0 or index.max() >= self.NC):
            raise IndexError(f"at_cells: column indices must lie in [0, {self.NC})")
        return self.flat("mean", ch)[:, index], self.flat("variance", ch)[:, index]

    # ---- merging
    def _same_layout(self, other: "CellRecord", what: str) -> None:
        if (other.blocks, other.dims, other.span_average) != (self.blocks, self.dims, self.span_average):
            raise ValueError(f"{what}: both records need the same blocks, dims and span_average")

    def _merged(self, sA, mA, cA, sB, mB, cB):
        nA, nB = (np.broadcast_to(s * self.column_n, (mA.shape[0], self.NC)) for s in (sA, sB))
        _, mean, cen = merge_moments(nA, np.moveaxis(mA, 1, 2), np.moveaxis(cA, 1, 2), nB, np.moveaxis(mB, 1, 2), np.moveaxis(cB, 1, 2),
                                     self.K, 2)
        return np.moveaxis(mean, 2, 1), np.moveaxis(cen, 2, 1)

    def merge(self, other: "CellRecord") -> "CellRecord":
        """Add ``other``'s samples (same blocks, options and batch size) to this record, env by env.  A record without a sample
        of its own takes ``other``'s state (a ``CellMoments`` puts it on the current device)."""
        self._same_layout(other, "merge")
        mB, cB = other._state()
        if self._unset():
            self._set_state(mB, cB)
            self.samples = other.samples
            return self
        mA, cA = self._state()
        if mA.shape != mB.shape:
            raise ValueError(f"merge: batch sizes differ, {mA.shape[0]} and {mB.shape[0]}")
        self._set_state(*self._merged(self.samples, mA, cA, other.samples, mB, cB))
        self.samples += other.samples
        return self

    def pooled(self) -> "HostCellMoments":
        """The envs of the batch merged into one ensemble record (``B = 1``, ``samples`` counts every env's), on the host in fp64."""
        mean, cen = self._state()
        am, ac = mean[:1], cen[:1]
        for b in range(1, mean.shape[0]):
            am, ac = self._merged(b * self.samples, am, ac, self.samples, mean[b:b + 1], cen[b:b + 1])
        return self._like(self.samples * mean.shape[0], am, ac)

    # ---- files (module docstring)
    def save(self, directory, pooled: bool = False) -> None:
        rec = self.pooled() if pooled else self
        mean, cen = rec._state()
        os.makedirs(directory, exist_ok=True)
        d, dirs = self.dims, []
        for b in range(mean.shape[0]):
            path = str(directory) if pooled else os.path.join(str(directory), "env_%04d" % b)
            os.makedirs(path, exist_ok=True)
            dirs.append("." if pooled else os.path.basename(path))
            np.savez_compressed(os.path.join(path, FILE_STATE), samples=np.asarray(rec.samples, np.int64), mean=mean[b], central=cen[b])
            for i in range(len(self.blocks)):
                n = np.asarray(rec.samples * int(self.table[i][2]), np.int64)
                m = rec._block(mean[b], i)                                      # [K, (nz,) ny, nx]
                c = rec._block(cen[b], i)
                diag = [self._pair(k, k) for k in range(self.K)]
                np.savez_compressed(os.path.join(path, f"block{i}_vel_stats.npz"), n=n, mean=m[:d], sum_squares=c[diag[:d]])
                np.savez_compressed(os.path.join(path, f"block{i}_p_stats.npz"), n=n, mean=m[d:], sum_squares=c[diag[d:]])
                for x in range(d):
                    for y in range(x + 1, d):
                        np.savez_compressed(os.path.join(path, f"block{i}_vel_cov_{self.channels[x]}{self.channels[y]}.npz"), n=n,
                                            mean_x=m[x:x + 1], mean_y=m[y:y + 1], C=c[self._pair(x, y)][None])
        meta = {"blocks": [[list(size), off] for size, off in self.blocks], "dims": d, "span_average": self.span_average,
                "pooled": bool(pooled), "dirs": dirs}
        with open(os.path.join(str(directory), FILE_META), "w") as f:
            json.dump(meta, f, indent=1)

    @staticmethod
    def load(directory) -> "HostCellMoments":
        """The record ``save`` wrote into ``directory`` (per env or pooled), bit for bit."""
        with open(os.path.join(str(directory), FILE_META)) as f:
            meta = json.load(f)
        r = HostCellMoments([(tuple(size), off) for size, off in meta["blocks"]], int(meta["dims"]), bool(meta["span_average"]))
        samples, means, cens = set(), [], []
        for d in meta["dirs"]:
            with np.load(os.path.join(str(directory), d, FILE_STATE)) as z:
                if z["mean"].shape != (r.K, r.NC) or z["central"].shape != (r.P, r.NC):
                    raise IOError(f"{d}/{FILE_STATE} does not hold {r.K} channels of {r.NC} columns")
                samples.add(int(z["samples"]))
                means.append(z["mean"])
                cens.append(z["central"])
        if len(samples) != 1:
            raise IOError(f"{directory}: the envs of a record hold the same number of samples, found {sorted(samples)}")
        r._set_state(np.stack(means), np.stack(cens))
        r.samples = samples.pop()
        return r


def _check_fields(rec: CellRecord, velocity, pressure, what: str) -> int:
    if velocity.ndim != 3 or velocity.shape[1] != rec.dims:
        raise ValueError(f"{what}: velocity must be the flat multi-block field [B, {rec.dims}, N], got {tuple(velocity.shape)}")
    B, _, N = (int(s) for s in velocity.shape)
    if tuple(pressure.shape) != (B, N):
        raise ValueError(f"{what}: pressure must be [B, N] = {(B, N)}, got {tuple(pressure.shape)}")
    if N < rec.min_cells:
        raise ValueError(f"{what}: the blocks need {rec.min_cells} cells, the fields hold {N}")
    return B


class HostCellMoments(CellRecord):
    """The NumPy fp64 twin of ``CellMoments``: same interface, same merge rule, arrays on the host."""

    def update(self, velocity, pressure) -> None:
        velocity, pressure = np.asarray(velocity), np.asarray(pressure)
        B = _check_fields(self, velocity, pressure, "HostCellMoments.update")
        v = np.concatenate([np.moveaxis(velocity, 1, 0), pressure[None]]).astype(np.float64)            # [K, B, N]
        mean, cen = sample_cell_moments(v, self.table)
        if self._mean is None:
            self._set_state(mean, cen)
        elif self._mean.shape[0] != B:
            raise ValueError("HostCellMoments.update: batch size changed between updates")
        else:
            self._set_state(*self._merged(self.samples, self._mean, self._central, 1, mean, cen))
        self.samples += 1


class CellMoments(CellRecord):
    """The GPU accumulator.  ``update(velocity, pressure)`` takes the domain's own flat tensors (float32 -> ``libfluidgym_hip.so``,
    float64 -> the fp64 library), reads them in place and runs one launch on the current stream."""

    def __init__(self, blocks, dims: int, span_average: bool = True):
        super().__init__(blocks, dims, span_average)
        self._dev = None        # (mean [B, K, NC], central [B, P, NC]) on the device
        self._table = (ctypes.c_int64 * self.table.size)(*self.table.reshape(-1).tolist())

    @classmethod
    def for_domain(cls, domain, span_average: bool = True) -> "CellMoments":
        """The accumulator of a prepared ``MultiBlockDomain``."""
        if not domain.prepared:
            raise RuntimeError("CellMoments.for_domain: PrepareSolve() the domain first (the cell offsets do not exist yet)")
        return cls([(b.size, b.cell_offset) for b in domain.blocks], domain.dims, span_average)

    def _unset(self) -> bool:
        return self._dev is None

    def _state(self):
        if self._dev is None:
            raise RuntimeError("no sample recorded yet")
        return tuple(t.cpu().numpy() for t in self._dev)

    def _set_state(self, mean, central) -> None:
        if self._dev is None:       # merge() into a record without a sample of its own: on the current device
            dev = torch.device("cuda", torch.cuda.current_device())
            self._dev = tuple(torch.empty(np.shape(v), dtype=torch.float64, device=dev) for v in (mean, central))
        for t, v in zip(self._dev, (mean, central)):
            t.copy_(torch.as_tensor(np.ascontiguousarray(v, np.float64)).reshape(t.shape))

    def update(self, velocity: torch.Tensor, pressure: torch.Tensor) -> None:
        what = "CellMoments.update"
        for t in (velocity, pressure):
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise ValueError(f"{what}: the fields must be tensors on the GPU (HostCellMoments takes host arrays)")
            if t.dtype != velocity.dtype or t.device != velocity.device:
                raise TypeError(f"{what}: both fields need one dtype and device")
            if not t.is_contiguous():
                raise ValueError(f"{what}: the fields are read in place and must be contiguous")
        if velocity.dtype not in (torch.float32, torch.float64):
            raise TypeError(f"{what}: float32 or float64 fields, got {velocity.dtype}")
        B = _check_fields(self, velocity, pressure, what)
        dev = velocity.device
        if self._dev is None:
            self._dev = (torch.empty(B, self.K, self.NC, dtype=torch.float64, device=dev),
                         torch.empty(B, self.P, self.NC, dtype=torch.float64, device=dev))
        elif self._dev[0].shape[0] != B or self._dev[0].device != dev:
            raise ValueError(f"{what}: batch size or device changed between updates")
        lib = F.library(velocity.dtype)
        mean, cen = self._dev
        with torch.cuda.device(dev):
            L.check(lib.fg_mb_cell_moments(F.ptr(velocity), F.ptr(pressure), self.dims, B, int(velocity.shape[2]), self._table,
                                           len(self.blocks), self.samples, F.ptr(mean), F.ptr(cen), F.stream_ptr(dev)), lib=lib)
        self.samples += 1
