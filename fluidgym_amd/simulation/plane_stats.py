"""Online plane-averaged flow statistics: mean profiles, Reynolds stresses, skewness and flatness per wall-normal row.

The reference accumulates these with ``WelfordOnlineParallel_Torch`` / ``CovarianceOnlineParallel_Torch`` /
``MultivariateMomentsOnlineParallel_Torch`` (``pict/data/online_statistics.py:31-266, 419-787``), fed by
``TCF_tools.VelocityStats.record_vel_stats`` (``:1480-1507``): statistics of ``u, v, w, p`` per row ``y``, averaged over the
homogeneous directions ``z, x`` and merged over the samples of a run.  Here one sample of a batch of ``B`` envs is one launch of
``fg_plane_moments`` (``csrc/fg_planestats.hip``) that leaves nothing on the host; every env is its own realisation, and
``pooled()`` merges them into one ensemble that converges ``B`` times sooner.

A record holds, per env, ``n`` (cells seen per row) and, per row, the ``K`` means and ``M`` central sums in the order of
``moment_keys``: the ``K (K + 1) / 2`` sums of ``d_i d_j`` (``i <= j``), from order 3 the ``K`` sums of ``d_i^3``, at order 4 the
``K`` sums of ``d_i^4`` (``d`` = deviation from the mean).  Two records merge by the pairwise update of Pebay et al. 2016 with
``delta = mean_B - mean_A``.  The reference's own merge takes ``delta`` the other way round and is off by 1e-2 of the sums in its
third- and fourth-order moments (its order-2 sums are right): for those orders the yardstick is a one-shot evaluation over all
samples.

``PlaneMoments`` accumulates on the GPU, ``HostPlaneMoments`` is its NumPy fp64 twin (the reference of the tests, usable where the
data already lives on the host).  Both share the accessors, ``merge`` / ``pooled``, the half-channel fold, the wall units of
``VelocityStats`` (``TCF_tools.py:462-482, 1465-1478, 1561-1620``) and ``save`` in the reference's file layouts.
"""
from __future__ import annotations

import json
import os
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from .. import _lib as L
from . import plane_fields as F

CHANNEL_SETS = (("u", "v", "p"), ("u", "v", "p", "T"), ("u", "v", "w", "p"), ("u", "v", "w", "p", "T"))
# file names of VelocityStats.save_vel_stats (TCF_tools.py:1764-1779)
FILE_VEL, FILE_P, FILE_COV, FILE_MOMENTS, FILE_META = ("online_stats_vel.npz", "online_stats_p.npz", "online_stats_vel_cov.npz",
                                                       "online_moments.npz", "plane_moments.json")


def moment_keys(K: int, order: int) -> List[Tuple[int, ...]]:
    """Exponent tuples of the central sums, in the order of the ``central`` array of ``fg_plane_moments``."""
    keys = []
    for i in range(K):
        for j in range(i, K):
            k = [0] * K
            k[i] += 1
            k[j] += 1
            keys.append(tuple(k))
    for o in range(3, order + 1):
        keys += [tuple(o if c == i else 0 for c in range(K)) for i in range(K)]
    return keys


def merge_moments(nA, meanA, cenA, nB, meanB, cenB, K: int, order: int):
    """Pairwise update (Pebay et al. 2016, without weights): ``n [...]``, ``mean [..., K]``, ``central [..., M]`` of A and B ->
    those of the union.  Where one side is empty (``n = 0``) the other is returned as it is."""
    nA, nB = np.asarray(nA, np.float64), np.asarray(nB, np.float64)
    meanA, meanB, cenA, cenB = (np.asarray(v, np.float64) for v in (meanA, meanB, cenA, cenB))
    n = nA + nB
    P = K * (K + 1) // 2
    with np.errstate(all="ignore"):
        dl = meanB - meanA
        mean = (nA[..., None] * meanA + nB[..., None] * meanB) / n[..., None]
        cen = np.empty(np.broadcast_shapes(cenA.shape, cenB.shape))
        q, diag = 0, {}
        for i in range(K):
            for j in range(i, K):
                if i == j:
                    diag[i] = q
                cen[..., q] = cenA[..., q] + cenB[..., q] + dl[..., i] * dl[..., j] * (nA * nB / n)
                q += 1
        for k in range(K if order >= 3 else 0):
            d, a2, b2 = dl[..., k], cenA[..., diag[k]], cenB[..., diag[k]]
            a3, b3 = cenA[..., P + k], cenB[..., P + k]
            cen[..., P + k] = a3 + b3 + d ** 3 * (nA * nB * (nA - nB) / (n * n)) + 3.0 * d * ((nA * b2 - nB * a2) / n)
            if order >= 4:
                cen[..., P + K + k] = (cenA[..., P + K + k] + cenB[..., P + K + k]
                                       + d ** 4 * (nA * nB * (nA * nA - nA * nB + nB * nB) / (n * n * n))
                                       + 6.0 * d * d * ((nA * nA * b2 + nB * nB * a2) / (n * n)) + 4.0 * d * ((nA * b3 - nB * a3) / n))
    eA, eB = (nA == 0)[..., None], (nB == 0)[..., None]
    mean = np.where(eA, meanB, np.where(eB, meanA, mean))
    cen = np.where(eA, cenB, np.where(eB, cenA, cen))
    return n, mean, cen


def sample_moments(values: np.ndarray, order: int):
    """One sample on the host: ``values [K, B, nz, ny, nx]`` -> ``n`` (scalar), ``mean [B, ny, K]``, ``central [B, ny, M]`` by two
    fp64 passes.  A row with a non-finite cell in any channel is NaN in every channel, as on the device."""
    v = np.asarray(values, np.float64)
    K = v.shape[0]
    cells = v.shape[2] * v.shape[4]
    with np.errstate(all="ignore"):
        mean = v.sum(axis=(2, 4)) / cells                                   # [K, B, ny]
        mean = np.where(np.isfinite(mean).all(axis=0, keepdims=True), mean, np.nan)
        d = v - mean[:, :, None, :, None]
        cen = [(np.prod([d[c] ** e for c, e in enumerate(key) if e], axis=0)).sum(axis=(1, 3)) for key in moment_keys(K, order)]
    return float(cells), np.moveaxis(mean, 0, -1).copy(), np.stack(cen, axis=-1)


class PlaneRecord(F.WallUnits):
    """Accessors, merging, wall units and files of a record ``n [B]``, ``mean [B, ny, K]``, ``central [B, ny, M]``; the two
    accumulators below say where the arrays live."""

    def __init__(self, channels: Sequence[str] = ("u", "v", "w", "p"), order: int = 2):
        channels = tuple(channels)
        if channels not in CHANNEL_SETS:
            raise ValueError(f"channels must be one of {CHANNEL_SETS}, got {channels}")
        if int(order) not in (2, 3, 4):
            raise ValueError(f"order must be 2, 3 or 4, got {order}")
        self.channels, self.order = channels, int(order)
        self.K = len(channels)
        self.keys = moment_keys(self.K, self.order)
        self.M = len(self.keys)
        self._index = {k: q for q, k in enumerate(self.keys)}

    # ---- where the arrays live: overridden by PlaneMoments
    def _state(self):
        if self._n is None:
            raise RuntimeError("no sample recorded yet")
        return self._n, self._mean, self._central

    def _set_state(self, n, mean, central) -> None:
        self._n, self._mean, self._central = (np.ascontiguousarray(v, np.float64) for v in (n, mean, central))

    _n = _mean = _central = None

    def _like(self, n, mean, central, channels=None) -> "HostPlaneMoments":
        r = HostPlaneMoments(channels or self.channels, self.order)
        r._set_state(n, mean, central)
        r.y_centers, r.viscosity = self.y_centers, self.viscosity
        return r

    def record(self) -> "HostPlaneMoments":
        """A host copy of the current state."""
        return self._like(*(np.array(v) for v in self._state()))

    # ---- accessors: [B, ny] each
    def _ch(self, ch: Union[int, str]) -> int:
        return self.channels.index(ch) if isinstance(ch, str) else int(ch)

    def _pure(self, ch, order: int) -> Tuple[int, ...]:
        c = self._ch(ch)
        return tuple(order if k == c else 0 for k in range(self.K))

    @property
    def n(self) -> np.ndarray:
        """Cells seen per row, ``[B]`` (every row of an env has seen the same number)."""
        return np.array(self._state()[0])

    def mean(self, ch) -> np.ndarray:
        return np.array(self._state()[1][..., self._ch(ch)])

    def moment(self, key) -> np.ndarray:
        """The central sum with exponents ``key`` (one per channel): ``n`` for order 0, 0 for order 1."""
        key = tuple(int(e) for e in key)
        if len(key) != self.K:
            raise KeyError(f"moment {key}: one exponent per channel {self.channels}")
        n, mean, cen = self._state()
        if sum(key) == 0:
            return np.broadcast_to(n[:, None], mean.shape[:2]).copy()
        if sum(key) == 1:
            return np.zeros(mean.shape[:2])
        if key not in self._index:
            raise KeyError(f"moment {key} is not recorded (order {self.order}: all second-order sums, pure third / fourth order)")
        return np.array(cen[..., self._index[key]])

    def moment_normalized(self, key) -> np.ndarray:
        return self.moment(key) / self._state()[0][:, None]

    def moment_standardized(self, ch, order: int) -> np.ndarray:
        """Skewness (``order`` 3) / flatness (4) of a channel: ``m_order / m_2^(order / 2)`` of the normalised moments."""
        with np.errstate(all="ignore"):
            return self.moment_normalized(self._pure(ch, order)) / self.moment_normalized(self._pure(ch, 2)) ** (order / 2)

    def variance(self, ch) -> np.ndarray:
        return self.moment_normalized(self._pure(ch, 2))

    def covariance(self, i, j) -> np.ndarray:
        key = [0] * self.K
        key[self._ch(i)] += 1
        key[self._ch(j)] += 1
        return self.moment_normalized(tuple(key))

    # ---- merging
    def merge(self, other: "PlaneRecord") -> "PlaneRecord":
        """Add ``other``'s samples (same channels, order, batch size and rows) to this record, env by env."""
        if (other.channels, other.order) != (self.channels, self.order):
            raise ValueError("merge: both records need the same channels and order")
        nB, mB, cB = other._state()
        if self._unset():
            self._set_state(nB, mB, cB)
            return self
        nA, mA, cA = self._state()
        if mA.shape != mB.shape:
            raise ValueError(f"merge: shapes differ, {mA.shape[:2]} and {mB.shape[:2]} (B, ny)")
        n, mean, cen = merge_moments(nA[:, None], mA, cA, nB[:, None], mB, cB, self.K, self.order)
        self._set_state(n[:, 0], mean, cen)
        return self

    def _unset(self) -> bool:
        return self._n is None

    def pooled(self) -> "HostPlaneMoments":
        """The envs of the batch merged into one ensemble record (``B = 1``), on the host in fp64."""
        n, mean, cen = self._state()
        an, am, ac = n[:1, None], mean[:1], cen[:1]
        for b in range(1, len(n)):
            an, am, ac = merge_moments(an, am, ac, n[b:b + 1, None], mean[b:b + 1], cen[b:b + 1], self.K, self.order)
        return self._like(an[:, 0], am, ac)

    def half_channel(self) -> "HostPlaneMoments":
        """Rows ``y`` and ``ny - 1 - y`` merged into ``ny // 2`` rows counted from the wall (``get_merged_half_avg_vel_stats``,
        TCF_tools.py:1561-1620).  The upper half is mirrored, so its wall-normal velocity changes sign: the mean of ``v``, every
        sum with an odd power of ``v`` (the reference flips the ``u v`` sum only and keeps the mean of ``v``)."""
        n, mean, cen = self._state()
        ny = mean.shape[1]
        h = ny // 2
        lo, up = slice(0, h), slice(ny - 1, ny - 1 - h, -1)
        iv = self.channels.index("v")
        sm = np.array([-1.0 if k == iv else 1.0 for k in range(self.K)])
        sc = np.array([-1.0 if key[iv] % 2 else 1.0 for key in self.keys])
        nn, m, c = merge_moments(n[:, None], mean[:, lo], cen[:, lo], n[:, None], mean[:, up] * sm, cen[:, up] * sc, self.K, self.order)
        r = self._like(nn[:, 0], m, c)
        r.y_centers = None if self.y_centers is None else np.asarray(self.y_centers)[:h]
        return r

    # ---- wall units: set_wall_units, _need_wall and u_wall of plane_fields.WallUnits
    def Re_wall(self) -> np.ndarray:
        return self.u_wall() / self._need_wall()[1]

    def to_wall_pos(self, coords, u_wall=None) -> np.ndarray:
        """``y+`` of coordinates in ``[-1, 1]``, ``[B, len(coords)]``."""
        uw = self.u_wall() if u_wall is None else np.atleast_1d(np.asarray(u_wall, np.float64))
        return (np.asarray(coords, np.float64)[None] + 1.0) * (uw[:, None] / self._need_wall()[1])

    def to_wall_vel(self, vel, order: int = 1, u_wall=None) -> np.ndarray:
        """A ``[B, ny]`` profile of velocity dimension ``order`` in wall units."""
        uw = self.u_wall() if u_wall is None else np.atleast_1d(np.asarray(u_wall, np.float64))
        return np.asarray(vel, np.float64) * (1.0 / uw[:, None] ** order)

    # ---- files: the layouts of the reference's save methods, one directory per env or one for the pooled record
    def save(self, directory, pooled: bool = False) -> None:
        """``pooled=True``: the ensemble record into ``directory``; else env ``b`` into ``directory/env_%04d``.  Per directory:
        ``WelfordOnlineParallel_Torch.save`` for velocity and pressure, ``CovarianceOnlineParallel_Torch.save`` for ``u, v``,
        ``MultivariateMomentsData.save`` for everything (``load`` reads that one), and the channel names in a JSON file."""
        rec = self.pooled() if pooled else self
        n, mean, cen = rec._state()
        os.makedirs(directory, exist_ok=True)
        vel = [k for k, c in enumerate(self.channels) if c in "uvw"]
        ip = self.channels.index("p")
        dirs = []
        for b in range(len(n)):
            d = str(directory) if pooled else os.path.join(str(directory), "env_%04d" % b)
            os.makedirs(d, exist_ok=True)
            dirs.append(os.path.basename(d) if not pooled else ".")
            nb = np.asarray(np.int64(n[b]) if float(n[b]).is_integer() else n[b])
            pure2 = [self._index[self._pure(k, 2)] for k in range(self.K)]
            np.savez_compressed(os.path.join(d, FILE_VEL), n=nb, mean=mean[b][:, vel].T[None],
                                sum_squares=cen[b][:, [pure2[k] for k in vel]].T[None])
            np.savez_compressed(os.path.join(d, FILE_P), n=nb, mean=mean[b, :, ip][None, None], sum_squares=cen[b, :, pure2[ip]][None, None])
            uv = tuple(1 if k < 2 else 0 for k in range(self.K))
            np.savez_compressed(os.path.join(d, FILE_COV), n=nb, mean_x=mean[b, :, 0][None, None], mean_y=mean[b, :, 1][None, None],
                                C=cen[b, :, self._index[uv]][None, None])
            data = {"channels": self.K, "n": nb, "num_means": self.K, "num_moments": self.M}
            for k in range(self.K):
                data["mean_%06d" % k] = mean[b, :, k][None, :, None]
            for q, key in enumerate(self.keys):
                data["moment_" + "_".join(str(e) for e in key)] = cen[b, :, q][None, :, None]
            np.savez_compressed(os.path.join(d, FILE_MOMENTS), **data)
        meta = {"channels": list(self.channels), "order": self.order, "pooled": bool(pooled), "dirs": dirs,
                "y_centers": None if self.y_centers is None else [float(v) for v in self.y_centers], "viscosity": self.viscosity}
        with open(os.path.join(str(directory), FILE_META), "w") as f:
            json.dump(meta, f, indent=1)

    @staticmethod
    def load(directory) -> "HostPlaneMoments":
        """The record ``save`` wrote into ``directory`` (per env or pooled), bit for bit."""
        with open(os.path.join(str(directory), FILE_META)) as f:
            meta = json.load(f)
        r = HostPlaneMoments(tuple(meta["channels"]), int(meta["order"]))
        ns, means, cens = [], [], []
        for d in meta["dirs"]:
            with np.load(os.path.join(str(directory), d, FILE_MOMENTS)) as z:
                if int(z["channels"]) != r.K or int(z["num_moments"]) != r.M:
                    raise IOError(f"{d}/{FILE_MOMENTS} does not hold {r.K} channels and {r.M} moments")
                ns.append(float(z["n"]))
                means.append(np.stack([z["mean_%06d" % k][0, :, 0] for k in range(r.K)], axis=-1))
                cens.append(np.stack([z["moment_" + "_".join(str(e) for e in key)][0, :, 0] for key in r.keys], axis=-1))
        r._set_state(np.array(ns), np.stack(means), np.stack(cens))
        if meta.get("y_centers") is not None:
            r.y_centers = np.asarray(meta["y_centers"], np.float64)
        r.viscosity = meta.get("viscosity")
        return r


def _gather(channels, velocity, pressure, scalar, what: str):
    """The moments record u, v(, w) and p of every field: a pressure always, ``w`` exactly in 3-D."""
    return F.gather(channels, velocity, pressure, scalar, what, pressure_required=True, w_exact=True)


class HostPlaneMoments(PlaneRecord):
    """The NumPy fp64 twin of ``PlaneMoments``: same interface, same merge rule, arrays on the host."""

    def update(self, velocity, pressure, scalar=None) -> None:
        velocity, pressure = np.asarray(velocity), np.asarray(pressure)
        scalar = None if scalar is None else np.asarray(scalar)
        fields = [np.asarray(t[:, c], np.float64) for t, c in _gather(self.channels, velocity, pressure, scalar, "HostPlaneMoments.update")]
        v = np.stack(fields)                                           # [K, B, (Z,) Y, X]
        if v.ndim == 4:
            v = v[:, :, None]
        cells, mean, cen = sample_moments(v, self.order)
        B = v.shape[1]
        if self._n is None:
            self._set_state(np.full(B, cells), mean, cen)
            return
        if self._mean.shape != mean.shape:
            raise ValueError("HostPlaneMoments.update: batch size or grid changed between updates")
        n, m, c = merge_moments(self._n[:, None], self._mean, self._central, np.full((B, 1), cells), mean, cen, self.K, self.order)
        self._set_state(n[:, 0], m, c)


class PlaneMoments(F.DeviceState, PlaneRecord):
    """The GPU accumulator.  ``update(velocity, pressure, scalar=None)`` takes the domain's own tensors (``[B, d, (Z,) Y, X]``,
    ``[B, 1, ...]``, ``[B, S, ...]``; float32 -> ``libfluidgym_hip.so``, float64 -> the fp64 library), reads their component slices in
    place and runs one launch on the current stream; nothing comes back to the host until an accessor is called."""

    _merge_into = "a HostPlaneMoments"
    # _dev: (n [B], mean [B, ny, K], central [B, ny, M], tickets [B]) on the device

    def _state(self):
        return self._read(3)

    def _set_state(self, n, mean, central) -> None:
        self._write(n, mean, central)

    def update(self, velocity: torch.Tensor, pressure: torch.Tensor, scalar: Optional[torch.Tensor] = None) -> None:
        what = "PlaneMoments.update"
        F.check_device_fields((velocity, pressure) + ((scalar,) if "T" in self.channels else ()), what, "HostPlaneMoments")
        parts = [(t.contiguous(), c) for t, c in _gather(self.channels, velocity, pressure, scalar, what)]
        B, nz, ny, nx = F.grid_of(velocity)
        dev = velocity.device
        if self._dev is None:
            self._shape = (B, nz, ny, nx, dev)
            self._dev = (torch.zeros(B, dtype=torch.float64, device=dev), torch.empty(B, ny, self.K, dtype=torch.float64, device=dev),
                         torch.empty(B, ny, self.M, dtype=torch.float64, device=dev), torch.zeros(B, dtype=torch.int64, device=dev))
        elif self._shape != (B, nz, ny, nx, dev):
            raise ValueError(f"{what}: batch size, grid or device changed between updates")
        ptrs, strides = F.channel_table(parts, nz * ny * nx)
        lib = F.library(velocity.dtype)
        n, mean, cen, tickets = self._dev
        with torch.cuda.device(dev):
            L.check(lib.fg_plane_moments(ptrs, strides, self.K, B, nz, ny, nx, self.order, F.ptr(n), F.ptr(mean), F.ptr(cen), F.ptr(tickets),
                                         F.stream_ptr(dev)), lib=lib)
