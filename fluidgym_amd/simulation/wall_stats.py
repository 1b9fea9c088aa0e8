"""Wall distributions of the multi-block domains (cylinder, airfoil) and their online statistics: per face of a closed wall the
wall-adjacent pressure ``p``, the wall shear stress ``tau_w`` and the traction ``fx, fy`` -- the integrand of the drag / lift sum --
and the time mean, variance and covariances of the four.

The reference sums the traction over the ring (``compute_forces_2d`` / ``_3d``, ``envs/util/forces.py:193-377``) and keeps no curve.
Here the curve of a batch of ``B`` envs is one launch of ``fg_mb_wall_distribution`` and one sample of its statistics one launch of
``fg_mb_wall_moments`` (``csrc/fg_wallstats.hip``) over the flat fields of a ``MultiBlockDomain``, gathered through the index tables
of a ``WallRing`` (``envs/forces.py``); nothing comes back to the host until an accessor is called.

A *face* is ``(layer, j)``: face ``j`` of the ring in spanwise layer ``layer`` (one layer in 2-D).  A *record* is face ``j`` over all
layers with ``span_average=True`` (``R = n`` records of ``n_B = layers`` faces per sample), one face otherwise (``R = layers * n``,
``n_B = 1``).  A ``WallRecord`` holds the number of merged samples and, per env and record, the four means and the ten sums of
``d_i d_j`` (``i <= j``, ``d`` = deviation from the mean) as ``mean [B, 4, R]`` and ``central [B, 10, R]``.  Records merge by the
order-2 rule of ``plane_stats.merge_moments`` (parallel Welford / Schubert-Gertz, ``delta = mean_B - mean_A``).

``sample_wall_faces`` is the NumPy twin of the device function: the same operations in the same order in the dtype asked for (the
kernel file is compiled without contraction, so the two agree to the bit wherever the division is correctly rounded).
``WallMoments`` accumulates on the GPU, ``HostWallMoments`` is its NumPy fp64 twin.  Both share the accessors, ``merge`` / ``pooled``
and the file.
"""
from __future__ import annotations

from typing import Tuple, Union

import numpy as np
import torch

from .. import _lib as L
from . import plane_fields as F
from .plane_stats import merge_moments

CHANNELS = ("p", "tau_w", "fx", "fy")
K = len(CHANNELS)
PAIRS = [(i, j) for i in range(K) for j in range(i, K)]
P = len(PAIRS)


def sample_wall_faces(u, ub, p, cell_index, slot_index, geom, viscosity, dtype, with_scale: bool = False):
    """The four channels of every wall face on the host, ``[B, 4, layers, n]`` in ``dtype``: ``u [B, d, N]``, ``ub [B, d, NB]``,
    ``p [B, N]`` (the flat fields), ``cell_index`` / ``slot_index [layers, n]``, ``geom [5, n]`` (normal x, normal y, tangential
    spacing, wall distance, face length: the packing of ``WallRing.forces``), ``viscosity`` a number or one per env ``[B]``.  The
    arithmetic of ``k_mb_wall_forces`` without the face length, operation by operation as ``ws_face`` of ``csrc/fg_wallstats.hip``
    does it.  ``with_scale``: also the sum of the absolute values of the terms every output is made of (what a rounding error
    of the chain is measured against), same shape."""
    dt_ = np.dtype(dtype)
    r = lambda v: np.asarray(v).astype(dt_)
    u, ub, p, geom = r(u), r(ub), r(p), r(geom)
    ci, si = np.asarray(cell_index, np.int64), np.asarray(slot_index, np.int64)
    if ci.ndim != 2 or ci.shape != si.shape or geom.shape != (5, ci.shape[1]):
        raise ValueError(f"index tables must be [layers, n] and geom [5, n], got {ci.shape}, {si.shape}, {geom.shape}")
    B = u.shape[0]
    nu = np.broadcast_to(r(viscosity).reshape(-1), (B,)) if np.ndim(viscosity) else np.full(B, viscosity, dt_)
    nu = nu.astype(dt_)[:, None, None]                                                       # [B, 1, 1]
    cl, cr = np.roll(ci, -1, axis=1), np.roll(ci, 1, axis=1)                                 # ci[j + 1 mod n], ci[j - 1 mod n]
    nx, ny, tl, wd = geom[0], geom[1], geom[2], geom[3]
    tx, ty = ny, -nx
    two, half = dt_.type(2), dt_.type(0.5)
    with np.errstate(all="ignore"):
        uc, ul, ur, uw, pc = u[:, :2][:, :, ci], u[:, :2][:, :, cl], u[:, :2][:, :, cr], ub[:, :2][:, :, si], p[:, ci]
        dn = (uc - uw) / wd                                                                  # [B, 2, layers, n]
        dt = (ur - ul) / (two * tl)
        du_dx, du_dy = dn[:, 0] * nx + dt[:, 0] * tx, dn[:, 0] * ny + dt[:, 0] * ty
        dv_dx, dv_dy = dn[:, 1] * nx + dt[:, 1] * tx, dn[:, 1] * ny + dt[:, 1] * ty
        sxy = half * (du_dy + dv_dx)
        two_nu = two * nu
        fx = (two_nu * du_dx - pc) * nx + two_nu * sxy * ny
        fy = two_nu * sxy * nx + (two_nu * dv_dy - pc) * ny
        tau = (two_nu * du_dx * nx + two_nu * sxy * ny) * ny - (two_nu * sxy * nx + two_nu * dv_dy * ny) * nx
        out = np.stack([pc, tau, fx, fy], axis=1).astype(dt_)
        if not with_scale:
            return out
        # the same expressions over absolute values, in fp64
        f8 = lambda v: np.abs(np.asarray(v, np.float64))
        anx, any_, nu8 = f8(nx), f8(ny), f8(two_nu)
        adn = (f8(uc) + f8(uw)) / f8(wd)
        adt = (f8(ur) + f8(ul)) / (2.0 * f8(tl))
        a_ux, a_uy = adn[:, 0] * anx + adt[:, 0] * any_, adn[:, 0] * any_ + adt[:, 0] * anx
        a_vx, a_vy = adn[:, 1] * anx + adt[:, 1] * any_, adn[:, 1] * any_ + adt[:, 1] * anx
        a_s = 0.5 * (a_uy + a_vx)
        s_fx = (nu8 * a_ux + f8(pc)) * anx + nu8 * a_s * any_
        s_fy = nu8 * a_s * anx + (nu8 * a_vy + f8(pc)) * any_
        s_tau = (nu8 * a_ux * anx + nu8 * a_s * any_) * any_ + (nu8 * a_s * anx + nu8 * a_vy * any_) * anx
    return out, np.stack([f8(pc), s_tau, s_fx, s_fy], axis=1)


def sample_wall_moments(faces: np.ndarray, span_average: bool) -> Tuple[np.ndarray, np.ndarray]:
    """One sample on the host: the channels ``faces [B, 4, layers, n]`` -> ``mean [B, 4, R]``, ``central [B, 10, R]`` by two fp64
    passes in ascending layer order, as the kernel takes them."""
    v = np.asarray(faces).astype(np.float64)
    B, _, layers, n = v.shape
    if not span_average:
        v = v.reshape(B, K, 1, layers * n)
    nl = v.shape[2]
    with np.errstate(all="ignore"):
        m = np.zeros((B, K, v.shape[3]))
        for l in range(nl):
            m = m + v[:, :, l]
        m = m / float(nl)
        d = v - m[:, :, None]
        cen = np.empty((B, P, v.shape[3]))
        for q, (i, j) in enumerate(PAIRS):
            c = np.zeros((B, v.shape[3]))
            for l in range(nl):
                c = c + d[:, i, l] * d[:, j, l]
            cen[:, q] = c
    return m, cen


class WallRecord:
    """Accessors, merging and the file of a record ``samples``, ``mean [B, 4, R]``, ``central [B, 10, R]`` of a ring of ``n`` faces
    in ``layers`` spanwise layers; the two accumulators below say where the arrays live."""

    channels = CHANNELS
    pairs = PAIRS

    def __init__(self, n: int, layers: int = 1, span_average: bool = True):
        if int(n) < 1 or int(layers) < 1:
            raise ValueError(f"n and layers must be positive, got {n}, {layers}")
        self.n_faces, self.layers, self.span_average = int(n), int(layers), bool(span_average)
        self.R = self.n_faces if self.span_average else self.layers * self.n_faces
        self.n_B = self.layers if self.span_average else 1                  # faces per record and sample
        self.shape = (self.n_faces,) if self.span_average or self.layers == 1 else (self.layers, self.n_faces)
        self.samples = 0

    # ---- where the arrays live: overridden by WallMoments
    _mean = _central = None

    def _state(self):
        if self._mean is None:
            raise RuntimeError("no sample recorded yet")
        return self._mean, self._central

    def _set_state(self, mean, central) -> None:
        self._mean, self._central = (np.ascontiguousarray(v, np.float64) for v in (mean, central))

    def _unset(self) -> bool:
        return self._mean is None

    def _like(self, samples: int, mean, central) -> "HostWallMoments":
        r = HostWallMoments(self.n_faces, self.layers, self.span_average)
        r._set_state(mean, central)
        r.samples = int(samples)
        return r

    def record(self) -> "HostWallMoments":
        """A host copy of the current state."""
        return self._like(self.samples, *(np.array(v) for v in self._state()))

    # ---- accessors: [B, n], without span averaging in 3-D [B, layers, n]
    def _ch(self, ch: Union[int, str]) -> int:
        return self.channels.index(ch) if isinstance(ch, str) else int(ch)

    def _pair(self, i, j) -> int:
        i, j = sorted((self._ch(i), self._ch(j)))
        return self.pairs.index((i, j))

    def _shaped(self, flat: np.ndarray) -> np.ndarray:
        return flat.reshape((flat.shape[0],) + self.shape)

    @property
    def count(self) -> float:
        """Faces every record has seen: ``samples * layers`` (``samples`` without span averaging)."""
        return float(self.samples * self.n_B)

    def mean(self, ch) -> np.ndarray:
        return self._shaped(np.array(self._state()[0][:, self._ch(ch)]))

    def covariance(self, i, j) -> np.ndarray:
        return self._shaped(self._state()[1][:, self._pair(i, j)] / self.count)

    def variance(self, ch) -> np.ndarray:
        return self.covariance(ch, ch)

    def rms(self, ch) -> np.ndarray:
        """The r.m.s. of the fluctuation: the square root of the variance."""
        return np.sqrt(np.maximum(self.variance(ch), 0.0))

    # ---- merging
    def _same_layout(self, other: "WallRecord", what: str) -> None:
        if (other.n_faces, other.layers, other.span_average) != (self.n_faces, self.layers, self.span_average):
            raise ValueError(f"{what}: both records need the same ring, layers and span_average")

    def _merged(self, sA, mA, cA, sB, mB, cB):
        nA, nB = (np.full((mA.shape[0], self.R), float(s * self.n_B)) for s in (sA, sB))
        _, mean, cen = merge_moments(nA, np.moveaxis(mA, 1, 2), np.moveaxis(cA, 1, 2), nB, np.moveaxis(mB, 1, 2), np.moveaxis(cB, 1, 2), K, 2)
        return np.moveaxis(mean, 2, 1), np.moveaxis(cen, 2, 1)

    def merge(self, other: "WallRecord") -> "WallRecord":
        """Add ``other``'s samples (same ring, options and batch size) to this record, env by env.  A record without a sample of its
        own takes ``other``'s state."""
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

    def pooled(self) -> "HostWallMoments":
        """The envs of the batch merged into one ensemble record (``B = 1``, ``samples`` counts every env's), on the host in fp64."""
        mean, cen = self._state()
        am, ac = mean[:1], cen[:1]
        for b in range(1, mean.shape[0]):
            am, ac = self._merged(b * self.samples, am, ac, self.samples, mean[b:b + 1], cen[b:b + 1])
        return self._like(self.samples * mean.shape[0], am, ac)

    # ---- the file: one .npz with the whole state
    def save(self, path) -> None:
        mean, cen = self._state()
        np.savez_compressed(path, samples=np.asarray(self.samples, np.int64), mean=mean, central=cen,
                            n=np.asarray(self.n_faces, np.int64), layers=np.asarray(self.layers, np.int64),
                            span_average=np.asarray(self.span_average), channels=np.asarray(self.channels))

    @staticmethod
    def load(path) -> "HostWallMoments":
        """The record ``save`` wrote, bit for bit."""
        with np.load(path) as z:
            r = HostWallMoments(int(z["n"]), int(z["layers"]), bool(z["span_average"]))
            if tuple(z["channels"]) != CHANNELS or z["mean"].shape[1:] != (K, r.R) or z["central"].shape[1:] != (P, r.R):
                raise IOError(f"{path} does not hold {K} channels of {r.R} wall records")
            r._set_state(z["mean"], z["central"])
            r.samples = int(z["samples"])
        return r


class HostWallMoments(WallRecord):
    """The NumPy fp64 twin of ``WallMoments``: ``update`` takes the channels of one sample ``[B, 4, layers, n]`` (of
    ``sample_wall_faces`` or of ``WallRing.distribution``); same merge rule, arrays on the host."""

    def update(self, faces) -> None:
        faces = np.asarray(faces)
        if faces.ndim != 4 or faces.shape[1:] != (K, self.layers, self.n_faces):
            raise ValueError(f"HostWallMoments.update: the channels must be [B, {K}, {self.layers}, {self.n_faces}], got {faces.shape}")
        mean, cen = sample_wall_moments(faces, self.span_average)
        if self._mean is None:
            self._set_state(mean, cen)
        elif self._mean.shape[0] != faces.shape[0]:
            raise ValueError("HostWallMoments.update: batch size changed between updates")
        else:
            self._set_state(*self._merged(self.samples, self._mean, self._central, 1, mean, cen))
        self.samples += 1


def check_wall_fields(domain, what: str):
    """The flat fields of a multi-block domain on the GPU, as the wall kernels read them in place: ``(velocity, boundary_velocity,
    pressure)``."""
    u, ub, p = domain.velocity, domain.boundary_velocity, domain.pressure
    F.check_device_fields((u, ub, p), what, "sample_wall_faces")
    if u.ndim != 3 or ub.ndim != 3 or p.ndim != 2 or ub.shape[:2] != u.shape[:2] or tuple(p.shape) != (u.shape[0], u.shape[2]):
        raise ValueError(f"{what}: needs the flat multi-block fields velocity [B, d, N], boundary_velocity [B, d, NB], pressure [B, N]")
    if not (u.is_contiguous() and ub.is_contiguous() and p.is_contiguous()):
        raise ValueError(f"{what}: the fields are read in place and must be contiguous")
    return u, ub, p


def wall_viscosity(viscosity, batch: int, like: torch.Tensor):
    """``(scalar, per-env tensor or None)`` of a viscosity given as a number or as one value per env."""
    if isinstance(viscosity, torch.Tensor) and viscosity.numel() > 1:
        if viscosity.numel() != batch:
            raise ValueError(f"viscosity must be a float or one value per env ({batch})")
        return 0.0, viscosity.detach().reshape(-1).to(device=like.device, dtype=like.dtype).contiguous()
    return float(viscosity), None


class WallMoments(WallRecord):
    """The GPU accumulator of one ring.  ``update(domain, viscosity)`` reads the domain's own flat tensors in place (float32 ->
    ``libfluidgym_hip.so``, float64 -> the fp64 library) and runs one launch on the current stream."""

    def __init__(self, cell_index: torch.Tensor, slot_index: torch.Tensor, geom: torch.Tensor, batch: int, span_average: bool = True):
        layers, n = (int(s) for s in cell_index.shape)
        super().__init__(n, layers, span_average)
        for t in (cell_index, slot_index):
            if t.dtype != torch.int32 or tuple(t.shape) != (layers, n) or not t.is_contiguous():
                raise ValueError("WallMoments: the index tables must be contiguous int32 [layers, n]")
        if tuple(geom.shape) != (5, n) or not geom.is_contiguous():
            raise ValueError("WallMoments: geom must be contiguous [5, n]")
        self._tables = (cell_index, slot_index, geom)
        self.batch = int(batch)
        self._dev = None        # (mean [B, 4, R], central [B, 10, R]) on the device

    @classmethod
    def for_ring(cls, ring, batch: int, dtype=torch.float32, span_average: bool = True) -> "WallMoments":
        """The accumulator of a ``WallRing`` for ``batch`` envs whose fields have ``dtype``."""
        return cls(*ring.native_tables(dtype), batch, span_average)

    def _unset(self) -> bool:
        return self._dev is None

    def _state(self):
        if self._dev is None:
            raise RuntimeError("no sample recorded yet")
        return tuple(t.cpu().numpy() for t in self._dev)

    def _set_state(self, mean, central) -> None:
        if self._dev is None:       # merge() into a record without a sample of its own: beside the ring's tables
            dev = self._tables[0].device
            self._dev = tuple(torch.empty(np.shape(v), dtype=torch.float64, device=dev) for v in (mean, central))
        for t, v in zip(self._dev, (mean, central)):
            t.copy_(torch.as_tensor(np.ascontiguousarray(v, np.float64)).reshape(t.shape))

    def update(self, domain, viscosity) -> None:
        what = "WallMoments.update"
        u, ub, p = check_wall_fields(domain, what)
        ci, si, geom = self._tables
        B, dev = int(u.shape[0]), u.device
        if B != self.batch or geom.dtype != u.dtype or geom.device != dev:
            raise ValueError(f"{what}: the accumulator was made for {self.batch} envs of {geom.dtype} on {geom.device}")
        if self._dev is None:
            self._dev = (torch.empty(B, K, self.R, dtype=torch.float64, device=dev), torch.empty(B, P, self.R, dtype=torch.float64, device=dev))
        nu, nu_B = wall_viscosity(viscosity, B, u)
        lib = F.library(u.dtype)
        mean, cen = self._dev
        with torch.cuda.device(dev):
            L.check(lib.fg_mb_wall_moments(F.ptr(u), F.ptr(ub), F.ptr(p), int(u.shape[1]), B, int(u.shape[2]), int(ub.shape[2]), F.ptr(ci),
                                           F.ptr(si), F.ptr(geom), self.n_faces, self.layers, nu, None if nu_B is None else F.ptr(nu_B),
                                           int(self.span_average), self.samples, F.ptr(mean), F.ptr(cen), F.stream_ptr(dev)), lib=lib)
        self.samples += 1
