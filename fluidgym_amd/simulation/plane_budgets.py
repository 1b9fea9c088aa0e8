"""Online Reynolds-stress budgets of channel flows: per wall-normal row the terms of the transport equation of ``<u_i' u_j'>`` --
production, dissipation, turbulent transport, viscous diffusion, velocity-pressure-gradient, forcing.

The reference accumulates them with ``TurbulentEnergyBudgetsOnlineParallel_Torch`` (``pict/data/online_statistics.py:790-1268``),
fed by ``VelocityStats`` next to the plane moments and the spectra (``TCF_tools.py:438-443, 1512-1516``): twelve full-field padded
differences and about fifty ``torch.mean`` / ``torch.sum`` passes per sample.  Here one sample of a batch of ``B`` envs is one launch
of ``fg_plane_budgets`` (``csrc/fg_planebudgets.hip``) that forms the gradients in registers and leaves nothing on the host.

A record holds, per env, ``n`` (cells seen per row) and, per row, the means of ``K`` channels and ``M`` central sums.  Channels:
``0..2`` ``u, v, w``; ``3..5`` ``dp/dx, dp/dy, dp/dz``; ``6 + 3 k + i`` ``d u_i / d x_k``; with forcing ``15..17`` ``s_x, s_y, s_z``
(``K`` = 15 or 18).  The central sums are named by ``budget_keys(forcing)``, tuples of channel indices (``M`` = 43 or 52).  Two records
merge by the pairwise update of Pebay et al. 2016 with ``delta = mean_B - mean_A``, mixed third-order sums included; the reference's
own merge of third-order sums is not right (see ``plane_stats``), so those are checked against a one-shot evaluation.

The gradient is the reference's ``_data_grad(borders="ZERO")``: a central difference over ``|pos[i + 1] - pos[i - 1]|`` with the ghost
position mirrored at both ends and the ghost value zero, on every axis; on y that ghost stands in for the wall.  On x and z the
further mode ``wrap`` takes the ghost value from the other end of the axis (the ghost distance stays the mirrored one, exact on a
uniform axis): the reference zero-pads its periodic directions too, which corrupts the first and last column of every plane, so the
envs use ``wrap`` on periodic faces and the zero mode exists to match the reference value for value.

Accumulation is in physical units.  ``as_wall=True`` scales at read-out: velocities by ``1 / u_wall`` each, lengths by
``u_wall / nu``, so that a budget term is scaled by ``nu / u_wall^4``.  The accessors keep the reference's formulas, which leave the
viscosity out of the dissipation and of the viscous diffusion (its coordinates are meant to be in wall units, where it is 1); in
wall units they carry it through the length scale, in physical units ``budget`` / ``residual`` multiply the two by ``viscosity``.

One deliberate departure: ``viscous_diffusion`` is the three-point second difference on the non-uniform rows (zero ghost, mirrored
ghost position).  The reference's ``_data_grad2`` computes its upper one-sided difference from the lower one
(``online_statistics.py:1101``) and is no second derivative once coordinates are given.

``PlaneBudgets`` accumulates on the GPU, ``HostPlaneBudgets`` is its NumPy fp64 twin.
"""
from __future__ import annotations

import json
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _lib as L
from . import plane_fields as F

K_BASE, K_FORCING = 15, 18
FILE_MOMENTS, FILE_GRAD, FILE_META = "budgets_moments.npz", "budgets_grad_%04d.npz", "plane_budgets.json"
# sign of a channel under the mirror y -> -y, v -> -v (half_channel): odd in v or in d/dy
_PARITY = [1, -1, 1, 1, -1, 1] + [(-1 if i == 1 else 1) * (-1 if k == 1 else 1) for k in range(3) for i in range(3)] + [1, -1, 1]


def channel_names(forcing: bool = False) -> List[str]:
    names = ["u", "v", "w", "dp/dx", "dp/dy", "dp/dz"] + ["d%s/d%s" % ("uvw"[i], "xyz"[k]) for k in range(3) for i in range(3)]
    return names + (["s_x", "s_y", "s_z"] if forcing else [])


def budget_keys(forcing: bool = False) -> List[Tuple[int, ...]]:
    """The central sums in the order of the ``central`` array of ``fg_plane_budgets``: tuples of ascending channel indices."""
    keys: List[Tuple[int, ...]] = [(i, j) for i in range(3) for j in range(i, 3)]
    keys += [(i, j, k) for i in range(3) for j in range(i, 3) for k in range(j, 3)]
    keys += [(i, 3 + j) for i in range(3) for j in range(3)]
    if forcing:
        keys += [(i, 15 + j) for i in range(3) for j in range(3)]
    for k in range(3):
        keys += [(6 + 3 * k + i, 6 + 3 * k + j) for i in range(3) for j in range(i, 3)]
    return keys


def _ghosted(pos) -> np.ndarray:
    pos = np.asarray(pos, np.float64)
    return np.concatenate([[2.0 * pos[0] - pos[1]], pos, [2.0 * pos[-1] - pos[-2]]])


def central_gradient(f, pos, axis: int, wrap: bool = False) -> np.ndarray:
    """``(f[i + 1] - f[i - 1]) / |pos[i + 1] - pos[i - 1]|`` along ``axis`` in fp64: mirrored ghost positions, ghost value 0 or,
    ``wrap``, the cell at the other end."""
    f = np.asarray(f, np.float64)
    lo, hi = np.roll(f, 1, axis), np.roll(f, -1, axis)
    if not wrap:
        first, last = [slice(None)] * f.ndim, [slice(None)] * f.ndim
        first[axis], last[axis] = slice(0, 1), slice(f.shape[axis] - 1, None)
        lo[tuple(first)] = 0.0
        hi[tuple(last)] = 0.0
    g = _ghosted(pos)
    shape = [1] * f.ndim
    shape[axis] = -1
    with np.errstate(all="ignore"):
        return (hi - lo) * (1.0 / np.abs(g[2:] - g[:-2])).reshape(shape)


def second_difference(f, pos, axis: int) -> np.ndarray:
    """The three-point second difference of ``f`` along ``axis`` on the points ``pos``, ghost value 0 at mirrored ghost positions:
    exact for a quadratic on interior points."""
    f = np.asarray(f, np.float64)
    pad = [(0, 0)] * f.ndim
    pad[axis] = (1, 1)
    fp = np.moveaxis(np.pad(f, pad), axis, -1)
    g = _ghosted(pos)
    hm, hp = g[1:-1] - g[:-2], g[2:] - g[1:-1]
    with np.errstate(all="ignore"):
        d2 = 2.0 * ((fp[..., 2:] - fp[..., 1:-1]) / hp - (fp[..., 1:-1] - fp[..., :-2]) / hm) / (hp + hm)
    return np.moveaxis(d2, -1, axis)


def budget_channels(velocity, pressure, source, x, y, z, wrap=(True, True)) -> List[np.ndarray]:
    """The ``K`` channel fields ``[B, Z, Y, X]`` (fp64) of one sample; the differences are taken of the values as they were cast."""
    v, p = np.asarray(velocity), np.asarray(pressure)
    f = [np.asarray(v[:, c], np.float64) for c in range(3)] + [np.asarray(p[:, 0], np.float64)]
    coords = ((x, 3, bool(wrap[0])), (y, 2, False), (z, 1, bool(wrap[1])))
    ch = f[:3] + [central_gradient(f[3], pos, ax, w) for pos, ax, w in coords]
    for pos, ax, w in coords:
        ch += [central_gradient(f[i], pos, ax, w) for i in range(3)]
    if source is not None:
        s = np.asarray(source)
        ch += [np.asarray(s[:, c], np.float64) for c in range(3)]
    return ch


def sample_budgets(channels: Sequence[np.ndarray], keys):
    """One sample on the host: channel fields ``[B, Z, Y, X]`` -> ``n`` (scalar), ``mean [B, ny, K]``, ``central [B, ny, M]`` by two
    fp64 passes.  A row with a non-finite value in any channel is NaN in every channel, as on the device."""
    v = np.stack(channels)                                                  # [K, B, Z, Y, X]
    cells = v.shape[2] * v.shape[4]
    with np.errstate(all="ignore"):
        mean = v.sum(axis=(2, 4)) / cells                                   # [K, B, ny]
        mean = np.where(np.isfinite(mean).all(axis=0, keepdims=True), mean, np.nan)
        d = v - mean[:, :, None, :, None]
        cen = []
        for key in keys:
            m = d[key[0]] * d[key[1]]
            if len(key) == 3:
                m = m * d[key[2]]
            cen.append(m.sum(axis=(1, 3)))
    return float(cells), np.moveaxis(mean, 0, -1).copy(), np.stack(cen, axis=-1)


def merge_budgets(nA, meanA, cenA, nB, meanB, cenB, keys):
    """Pairwise update (Pebay et al. 2016, without weights) of ``n [...]``, ``mean [..., K]``, ``central [..., M]``: for a third-order
    sum ``M_ijk = A + B + d_i d_j d_k nA nB (nA - nB) / n^2 + [d_i (nA B_jk - nB A_jk) + d_j (nA B_ik - nB A_ik)
    + d_k (nA B_ij - nB A_ij)] / n``.  Where one side is empty (``n = 0``) the other is returned as it is."""
    nA, nB = np.asarray(nA, np.float64), np.asarray(nB, np.float64)
    meanA, meanB, cenA, cenB = (np.asarray(v, np.float64) for v in (meanA, meanB, cenA, cenB))
    index = {k: q for q, k in enumerate(keys)}
    n = nA + nB
    with np.errstate(all="ignore"):
        dl = meanB - meanA
        mean = (nA[..., None] * meanA + nB[..., None] * meanB) / n[..., None]
        cen = np.empty(np.broadcast_shapes(cenA.shape, cenB.shape))
        w2, w3 = nA * nB / n, nA * nB * (nA - nB) / (n * n)
        for q, key in enumerate(keys):
            if len(key) == 2:
                cen[..., q] = cenA[..., q] + cenB[..., q] + dl[..., key[0]] * dl[..., key[1]] * w2
            else:
                i, j, k = key
                cross = 0.0
                for a, pair in ((i, (j, k)), (j, (i, k)), (k, (i, j))):
                    p = index[pair]
                    cross = cross + dl[..., a] * (nA * cenB[..., p] - nB * cenA[..., p])
                cen[..., q] = cenA[..., q] + cenB[..., q] + dl[..., i] * dl[..., j] * dl[..., k] * w3 + cross / n
    eA, eB = (nA == 0)[..., None], (nB == 0)[..., None]
    mean = np.where(eA, meanB, np.where(eB, meanA, mean))
    cen = np.where(eA, cenB, np.where(eB, cenA, cen))
    return n, mean, cen


class BudgetRecord(F.WallUnits):
    """Accessors, merging, wall units and files of a record ``n [B]``, ``mean [B, ny, K]``, ``central [B, ny, M]`` on the rows
    ``y``; the two accumulators below say where the arrays live.  Indices ``i, j, k`` are 0..2; every accessor returns ``[B, ny]``."""

    def __init__(self, x, y, z, forcing: bool = False, wrap: Tuple[bool, bool] = (True, True)):
        self.x, self.y, self.z = (np.array(c, np.float64).reshape(-1) for c in (x, y, z))
        for name, c in (("x", self.x), ("y", self.y), ("z", self.z)):
            if len(c) < 2 or not (np.all(np.diff(c) > 0) or np.all(np.diff(c) < 0)):
                raise ValueError(f"{name}: at least two strictly monotonic cell-centre coordinates, got {c}")
        self.forcing = bool(forcing)
        self.wrap = (bool(wrap[0]), bool(wrap[1]))
        self.K = K_FORCING if self.forcing else K_BASE
        self.keys = budget_keys(self.forcing)
        self.M = len(self.keys)
        self._index = {k: q for q, k in enumerate(self.keys)}

    # ---- where the arrays live: overridden by PlaneBudgets
    _n = _mean = _central = None

    def _state(self):
        if self._n is None:
            raise RuntimeError("no sample recorded yet")
        return self._n, self._mean, self._central

    def _set_state(self, n, mean, central) -> None:
        self._n, self._mean, self._central = (np.ascontiguousarray(v, np.float64) for v in (n, mean, central))

    def _unset(self) -> bool:
        return self._n is None

    def _like(self, n, mean, central, y=None) -> "HostPlaneBudgets":
        r = HostPlaneBudgets(self.x, self.y if y is None else y, self.z, self.forcing, self.wrap)
        r._set_state(n, mean, central)
        r.y_centers, r.viscosity = self.y_centers, self.viscosity
        return r

    def record(self) -> "HostPlaneBudgets":
        """A host copy of the current state."""
        return self._like(*(np.array(v) for v in self._state()))

    # ---- wall units: set_wall_units, _need_wall and u_wall of plane_fields.WallUnits
    _u_wall_fixed: Optional[np.ndarray] = None            # set by half_channel(): the fold has lost the upper wall

    def _scale(self, vel_order: int, derivatives: int, as_wall: bool):
        """The wall-unit factor ``[B, 1]`` of a quantity of ``vel_order`` velocities and ``derivatives`` inverse lengths."""
        if not as_wall:
            return 1.0
        uw = self._u_wall_fixed if self._u_wall_fixed is not None else self.u_wall()
        return (uw ** -float(vel_order) * (self._need_wall()[1] / uw) ** derivatives)[:, None]

    # ---- accessors
    @property
    def n(self) -> np.ndarray:
        """Cells seen per row, ``[B]``."""
        return np.array(self._state()[0])

    def channel_mean(self, c: int) -> np.ndarray:
        """The mean of channel ``c`` (``channel_names``), physical units."""
        return np.array(self._state()[1][..., int(c)])

    def central_sum(self, key) -> np.ndarray:
        """The central sum of the channels ``key`` (any order of a tuple of ``budget_keys``), physical units."""
        key = tuple(sorted(int(c) for c in key))
        if key not in self._index:
            raise KeyError(f"central sum {key} is not recorded (budget_keys)")
        return np.array(self._state()[2][..., self._index[key]])

    def _normalized(self, key) -> np.ndarray:
        return self.central_sum(key) / self._state()[0][:, None]

    @staticmethod
    def _vel(*idx):
        for i in idx:
            if int(i) not in (0, 1, 2):
                raise IndexError(f"velocity / direction index {i} outside 0..2")
        return tuple(int(i) for i in idx)

    def mean(self, i, as_wall: bool = False) -> np.ndarray:
        (i,) = self._vel(i)
        return self.channel_mean(i) * self._scale(1, 0, as_wall)

    def mean_grad(self, i, grad_dim, as_wall: bool = False) -> np.ndarray:
        """``d<u_i>/dx_k``: zero along the averaged directions x and z, as in the reference; along y the recorded mean of ``du_i/dy``."""
        i, k = self._vel(i, grad_dim)
        if k != 1:
            return np.zeros(self._state()[1].shape[:2])
        return self.channel_mean(6 + 3 * k + i) * self._scale(1, 1, as_wall)

    def covariance(self, i, j, as_wall: bool = False) -> np.ndarray:
        return self._normalized(self._vel(i, j)) * self._scale(2, 0, as_wall)

    def covariance_grad(self, i, j, grad_dim, as_wall: bool = False) -> np.ndarray:
        i, j, k = self._vel(i, j, grad_dim)
        return self._normalized((6 + 3 * k + i, 6 + 3 * k + j)) * self._scale(2, 2, as_wall)

    def skewness(self, i, j, k, as_wall: bool = False) -> np.ndarray:
        """The normalised third-order moment ``<u_i' u_j' u_k'>`` (the reference's name for it)."""
        return self._normalized(self._vel(i, j, k)) * self._scale(3, 0, as_wall)

    def production(self, i, j, as_wall: bool = False) -> np.ndarray:
        return (-self.covariance(i, 1, as_wall) * self.mean_grad(j, 1, as_wall)
                - self.covariance(j, 1, as_wall) * self.mean_grad(i, 1, as_wall))

    def dissipation(self, i, j, as_wall: bool = False) -> np.ndarray:
        """``2 sum_k <d_k u_i' d_k u_j'>``, without the viscosity (module docstring)."""
        return 2.0 * ((self.covariance_grad(i, j, 0, as_wall) + self.covariance_grad(i, j, 1, as_wall)) + self.covariance_grad(i, j, 2, as_wall))

    def turbulent_transport(self, i, j, as_wall: bool = False) -> np.ndarray:
        """``-d<u_i' u_j' v'>/dy``: the zero-ghost central difference of the triple-moment profile on the rows, fp64 on the host."""
        return -central_gradient(self.skewness(i, j, 1), self.y, 1) * self._scale(3, 1, as_wall)

    def viscous_diffusion(self, i, j, as_wall: bool = False) -> np.ndarray:
        """``d^2<u_i' u_j'>/dy^2`` without the viscosity: the three-point second difference on the non-uniform rows, zero ghost.
        NOT the reference's ``_data_grad2``, which is no second derivative when coordinates are given (module docstring)."""
        return second_difference(self.covariance(i, j), self.y, 1) * self._scale(2, 2, as_wall)

    def velocity_pressure_gradient(self, i, j, as_wall: bool = False) -> np.ndarray:
        i, j = self._vel(i, j)
        return -(self._normalized((i, 3 + j)) + self._normalized((j, 3 + i))) * self._scale(3, 1, as_wall)

    def velocity_forcing(self, i, j, as_wall: bool = False) -> np.ndarray:
        if not self.forcing:
            raise RuntimeError("Forcing moments are not tracked.")
        i, j = self._vel(i, j)
        return (self._normalized((i, 15 + j)) + self._normalized((j, 15 + i))) * self._scale(3, 1, as_wall)

    def budget(self, i, j, as_wall: bool = False) -> Dict[str, np.ndarray]:
        """All terms of the ``<u_i' u_j'>`` equation.  In wall units the accessors' values; in physical units the dissipation and the
        viscous diffusion times ``viscosity`` (which then has to be set)."""
        nu = 1.0
        if not as_wall:
            if self.viscosity is None:
                raise RuntimeError("budget in physical units needs the viscosity: set_wall_units(y_centers, viscosity)")
            nu = self.viscosity
        out = {"production": self.production(i, j, as_wall), "dissipation": nu * self.dissipation(i, j, as_wall),
               "turbulent_transport": self.turbulent_transport(i, j, as_wall), "viscous_diffusion": nu * self.viscous_diffusion(i, j, as_wall),
               "velocity_pressure_gradient": self.velocity_pressure_gradient(i, j, as_wall)}
        if self.forcing:
            out["velocity_forcing"] = self.velocity_forcing(i, j, as_wall)
        return out

    def residual(self, i, j, as_wall: bool = False) -> np.ndarray:
        """The signed sum of ``budget(i, j)``: every term enters with ``+`` but the dissipation; 0 for a converged record."""
        b = self.budget(i, j, as_wall)
        return sum(-v if name == "dissipation" else v for name, v in b.items())

    # ---- merging
    def _same(self, other: "BudgetRecord") -> bool:
        return (other.forcing == self.forcing and other.wrap == self.wrap
                and all(np.array_equal(a, b) for a, b in ((self.x, other.x), (self.y, other.y), (self.z, other.z))))

    def merge(self, other: "BudgetRecord") -> "BudgetRecord":
        """Add ``other``'s samples (same grid, forcing, border mode and batch size) to this record, env by env."""
        if not self._same(other):
            raise ValueError("merge: both records need the same coordinates, forcing flag and border mode")
        nB, mB, cB = other._state()
        if self._unset():
            self._set_state(nB, mB, cB)
            return self
        nA, mA, cA = self._state()
        if mA.shape != mB.shape:
            raise ValueError(f"merge: shapes differ, {mA.shape[:2]} and {mB.shape[:2]} (B, ny)")
        n, mean, cen = merge_budgets(nA[:, None], mA, cA, nB[:, None], mB, cB, self.keys)
        self._set_state(n[:, 0], mean, cen)
        return self

    def pooled(self) -> "HostPlaneBudgets":
        """The envs of the batch merged into one ensemble record (``B = 1``), on the host in fp64."""
        n, mean, cen = self._state()
        an, am, ac = n[:1, None], mean[:1], cen[:1]
        for b in range(1, len(n)):
            an, am, ac = merge_budgets(an, am, ac, n[b:b + 1, None], mean[b:b + 1], cen[b:b + 1], self.keys)
        return self._like(an[:, 0], am, ac)

    def half_channel(self) -> "HostPlaneBudgets":
        """Rows ``y`` and ``ny - 1 - y`` merged into ``ny // 2`` rows counted from the wall.  The upper half is mirrored, so every
        mean and every sum with an odd count of ``v`` or ``d/dy`` changes sign.  The friction velocity is kept from the full record;
        the last row of ``turbulent_transport`` / ``viscous_diffusion`` of the fold sees a zero ghost at the centreline, not a wall."""
        n, mean, cen = self._state()
        ny = mean.shape[1]
        h = ny // 2
        lo, up = slice(0, h), slice(ny - 1, ny - 1 - h, -1)
        sm = np.array(_PARITY[:self.K], np.float64)
        sc = np.array([np.prod([_PARITY[c] for c in key]) for key in self.keys], np.float64)
        nn, m, c = merge_budgets(n[:, None], mean[:, lo], cen[:, lo], n[:, None], mean[:, up] * sm, cen[:, up] * sc, self.keys)
        r = self._like(nn[:, 0], m, c, y=self.y[:h] if h >= 2 else self.y[:2])
        if self.y_centers is not None and self.viscosity is not None and len(self.y_centers) == ny:
            r._u_wall_fixed = self.u_wall()
        r.y_centers = None if self.y_centers is None else np.asarray(self.y_centers)[:h]
        return r

    # ---- files: the layout of TurbulentEnergyBudgetsOnlineParallel_Torch.save, one directory per env or one for the pooled record
    def _file_tables(self):
        """Per file the channels it holds (in the file's own order): the moments file u, v, w, dp/dx_j (, s_j), a gradient file
        ``d_k u, d_k v, d_k w``."""
        files = [(FILE_MOMENTS, list(range(6)) + ([15, 16, 17] if self.forcing else []))]
        return files + [(FILE_GRAD % k, [6 + 3 * k + i for i in range(3)]) for k in range(3)]

    def save(self, directory, pooled: bool = False) -> None:
        """``pooled=True``: the ensemble record into ``directory``; else env ``b`` into ``directory/env_%04d``.  Per directory
        ``budgets_moments.npz`` and ``budgets_grad_0000.npz`` .. ``budgets_grad_0002.npz`` with the keys of
        ``MultivariateMomentsData.save``; coordinates, viscosity and the forcing flag in a JSON file beside them."""
        rec = self.pooled() if pooled else self
        n, mean, cen = rec._state()
        os.makedirs(directory, exist_ok=True)
        dirs = []
        for b in range(len(n)):
            d = str(directory) if pooled else os.path.join(str(directory), "env_%04d" % b)
            os.makedirs(d, exist_ok=True)
            dirs.append("." if pooled else os.path.basename(d))
            nb = np.asarray(np.int64(n[b]) if float(n[b]).is_integer() else n[b])
            for name, chans in self._file_tables():
                held = [(q, key) for q, key in enumerate(self.keys) if all(c in chans for c in key)]
                data = {"channels": len(chans), "n": nb, "num_means": len(chans), "num_moments": len(held)}
                for pos, c in enumerate(chans):
                    data["mean_%06d" % pos] = mean[b, :, c][None, :, None]
                for q, key in held:
                    e = [sum(1 for c in key if c == ch) for ch in chans]
                    data["moment_" + "_".join(str(v) for v in e)] = cen[b, :, q][None, :, None]
                np.savez_compressed(os.path.join(d, name), **data)
        meta = {"forcing": self.forcing, "wrap": list(self.wrap), "pooled": bool(pooled), "dirs": dirs,
                "x": [float(v) for v in self.x], "y": [float(v) for v in rec.y], "z": [float(v) for v in self.z],
                "y_centers": None if self.y_centers is None else [float(v) for v in self.y_centers], "viscosity": self.viscosity}
        with open(os.path.join(str(directory), FILE_META), "w") as f:
            json.dump(meta, f, indent=1)

    @staticmethod
    def load(directory) -> "HostPlaneBudgets":
        """The record ``save`` wrote into ``directory`` (per env or pooled), bit for bit."""
        with open(os.path.join(str(directory), FILE_META)) as f:
            meta = json.load(f)
        r = HostPlaneBudgets(meta["x"], meta["y"], meta["z"], bool(meta["forcing"]), tuple(meta["wrap"]))
        ny = len(r.y)
        ns, means, cens = [], [], []
        for d in meta["dirs"]:
            mean, cen = np.empty((ny, r.K)), np.empty((ny, r.M))
            for name, chans in r._file_tables():
                with np.load(os.path.join(str(directory), d, name)) as z:
                    if int(z["channels"]) != len(chans):
                        raise IOError(f"{d}/{name} does not hold {len(chans)} channels")
                    n = float(z["n"])
                    for pos, c in enumerate(chans):
                        mean[:, c] = z["mean_%06d" % pos][0, :, 0]
                    for q, key in enumerate(r.keys):
                        if all(c in chans for c in key):
                            e = [sum(1 for c in key if c == ch) for ch in chans]
                            cen[:, q] = z["moment_" + "_".join(str(v) for v in e)][0, :, 0]
            ns.append(n)
            means.append(mean)
            cens.append(cen)
        r._set_state(np.array(ns), np.stack(means), np.stack(cens))
        if meta.get("y_centers") is not None:
            r.y_centers = np.asarray(meta["y_centers"], np.float64)
        r.viscosity = meta.get("viscosity")
        return r

    # ---- argument checks shared by the two accumulators
    def _check_fields(self, velocity, pressure, source, what: str):
        if velocity.ndim != 5 or velocity.shape[1] != 3:
            raise ValueError(f"{what}: velocity must be [B, 3, Z, Y, X]; 2-D and multi-block domains are not supported")
        shape = tuple(int(s) for s in velocity.shape)
        if tuple(shape[2:]) != (len(self.z), len(self.y), len(self.x)):
            raise ValueError(f"{what}: the grid {shape[2:]} does not fit the coordinates ({len(self.z)}, {len(self.y)}, {len(self.x)}) (Z, Y, X)")
        if pressure is None or tuple(pressure.shape) != (shape[0], 1) + shape[2:]:
            raise ValueError(f"{what}: pressure must be [B, 1, Z, Y, X] on the velocity's grid")
        if self.forcing and (source is None or tuple(source.shape) != shape):
            raise ValueError(f"{what}: a record with forcing needs the velocity source [B, 3, Z, Y, X]")
        return shape


class HostPlaneBudgets(BudgetRecord):
    """The NumPy fp64 twin of ``PlaneBudgets``: same gradients, same two passes, same merge rule, arrays on the host."""

    def update(self, velocity, pressure, source=None) -> None:
        velocity, pressure = np.asarray(velocity), np.asarray(pressure)
        source = None if (source is None or not self.forcing) else np.asarray(source)
        B = self._check_fields(velocity, pressure, source, "HostPlaneBudgets.update")[0]
        ch = budget_channels(velocity, pressure, source, self.x, self.y, self.z, self.wrap)
        cells, mean, cen = sample_budgets(ch, self.keys)
        if self._n is None:
            self._set_state(np.full(B, cells), mean, cen)
            return
        if self._mean.shape != mean.shape:
            raise ValueError("HostPlaneBudgets.update: batch size or grid changed between updates")
        n, m, c = merge_budgets(self._n[:, None], self._mean, self._central, np.full((B, 1), cells), mean, cen, self.keys)
        self._set_state(n[:, 0], m, c)


class PlaneBudgets(F.DeviceState, BudgetRecord):
    """The GPU accumulator.  ``update(velocity, pressure, source=None)`` takes the domain's own tensors (``[B, 3, Z, Y, X]``,
    ``[B, 1, Z, Y, X]``, ``[B, 3, Z, Y, X]``; float32 -> ``libfluidgym_hip.so``, float64 -> the fp64 library), reads their component
    slices in place and runs one launch on the current stream; nothing comes back to the host until an accessor is called."""

    _merge_into = "a HostPlaneBudgets"
    # _dev: (n [B], mean [B, ny, K], central [B, ny, M], tickets [B], x, y, z) on the device

    def _state(self):
        return self._read(3)

    def _set_state(self, n, mean, central) -> None:
        self._write(n, mean, central)

    def update(self, velocity: torch.Tensor, pressure: torch.Tensor, source: Optional[torch.Tensor] = None) -> None:
        what = "PlaneBudgets.update"
        if not self.forcing:
            source = None
        F.check_device_fields((velocity, pressure) + ((source,) if self.forcing else ()), what, "HostPlaneBudgets")
        B, _, nz, ny, nx = self._check_fields(velocity, pressure, source, what)
        dev = velocity.device
        if self._dev is None:
            self._shape = (B, nz, ny, nx, dev)
            f64 = dict(dtype=torch.float64, device=dev)
            self._dev = (torch.zeros(B, **f64), torch.empty(B, ny, self.K, **f64), torch.empty(B, ny, self.M, **f64),
                         torch.zeros(B, dtype=torch.int64, device=dev)) + tuple(torch.as_tensor(c).to(**f64) for c in (self.x, self.y, self.z))
        elif self._shape != (B, nz, ny, nx, dev):
            raise ValueError(f"{what}: batch size, grid or device changed between updates")
        vel, prs = velocity.contiguous(), pressure.contiguous()
        parts = [(vel, 0), (vel, 1), (vel, 2), (prs, 0)]
        if self.forcing:
            src = source.contiguous()
            parts += [(src, 0), (src, 1), (src, 2)]
        ptrs, strides = F.channel_table(parts, nz * ny * nx)
        lib = F.library(velocity.dtype)
        n, mean, cen, tickets, dx, dy, dz = self._dev
        with torch.cuda.device(dev):
            L.check(lib.fg_plane_budgets(ptrs, strides, len(parts), B, nz, ny, nx, F.ptr(dx), F.ptr(dy), F.ptr(dz), int(self.wrap[0]),
                                         int(self.wrap[1]), F.ptr(n), F.ptr(mean), F.ptr(cen), F.ptr(tickets), F.stream_ptr(dev)), lib=lib)
