"""Point probes and Lagrangian tracers of a single-block domain on the GPU (``csrc/fg_tracers.hip``).

Both rest on one interpolant of the cell-centred fields of the block's stretched rectilinear grid.  Per axis there is a node array in
the dtype of the fields, built once from ``Block.edges`` in fp64 and then rounded:

* a periodic axis has the ``n`` cell centres as nodes; a position is wrapped into ``[lo, lo + L)`` and the interval between the last
  and the first centre spans the seam;
* a FIXED axis has ``n + 2`` nodes, the low face, the centres and the high face; a position is clamped to ``[lo, hi]``.

The value at a point is the multilinear blend of the ``2^d`` surrounding nodes (``a + w (b - a)`` per axis, ``b`` itself at
``w == 1``).  A centre node reads the field; a face node reads, for the velocity, the boundary velocity of that face (the first
axis in the order y, x, z at an edge or corner of the box) and, for the pressure and the scalar, the adjacent cell.

``sample_points`` reads fields at physical positions; ``TracerCloud`` moves particles with the flow: ``advect(dt)`` runs ``substeps``
midpoint steps in the velocity field as it stands (the field is frozen during a call: first order in ``dt`` for an unsteady flow,
second order in ``dt / substeps`` for a steady one), wraps at periodic seams, clamps at walls and respawns at the faces named in
``respawn_faces``.  An env's tracers read that env's fields alone, and there is no floating-point atomic: a result depends neither
on the batch nor on the launch order and repeats bit for bit.

Not here: drawing tracers into ``render_frames``, inertial particles, interpolation of the velocity in time between sim steps.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence

import numpy as np
import torch

from .. import _lib as L
from . import plane_fields as F
from .domain import Domain, face_index
from .state_bank import normalize_envs

FIELD_NAMES = ("u", "v", "w", "p", "T")
MAX_EXTRA = 8


def require_single_block(domain, what: str) -> None:
    if not isinstance(domain, Domain):
        raise NotImplementedError(f"{what} needs a single-block domain (RBC, TCF, channel envs); multi-block domains have no "
                                  "rectilinear node arrays")
    if domain.solver is None:
        raise RuntimeError(f"{what}: PrepareSolve() the domain first")


def node_arrays(edges, periodic, np_dtype):
    """Per axis ``(nodes, lo, length)``: the centres (periodic) or low face, centres, high face (FIXED), computed in fp64 from the
    vertex coordinates ``edges`` and rounded to ``np_dtype``."""
    out = []
    for e, per in zip(edges, periodic):
        e = np.asarray(e, np.float64)
        c = 0.5 * (e[1:] + e[:-1])
        nodes = c if per else np.concatenate([e[:1], c, e[-1:]])
        out.append((nodes.astype(np_dtype), np_dtype(e[0]), np_dtype(e[-1] - e[0])))
    return out


def default_fields(domain) -> tuple:
    return ("u", "v") + (("w",) if domain.dims == 3 else ()) + ("p",) + (("T",) if domain.n_scalars > 0 else ())


def requested_fields(fields, default, names, dims: int):
    """The field-name check and the column selection of a ``sample`` (here and in ``mb_tracers.MbPointMesh``): ``(extras, pick)`` --
    the cell-only fields among ``fields`` (``default`` for None) that the launch gathers after the ``dims`` velocity components, in
    the order of their first mention, and ``pick(out)``, which brings the launch's ``[B, P, dims + len(extras)]`` into the order of
    ``fields`` (``out`` itself where that is its order)."""
    fields = default if fields is None else tuple(fields)
    if not fields or any(f not in names for f in fields) or ("w" in fields and dims != 3):
        raise ValueError(f"fields must be names from {names} that fit the {dims}-D domain, got {fields}")
    extras = [f for f in dict.fromkeys(fields) if f not in ("u", "v", "w")]
    column = {"u": 0, "v": 1, "w": 2, **{name: dims + i for i, name in enumerate(extras)}}
    cols = [column[f] for f in fields]
    if cols == list(range(dims + len(extras))):
        return extras, lambda out: out
    return extras, lambda out: out.index_select(2, torch.as_tensor(cols, dtype=torch.int64, device=out.device))


class PointGrid:
    """The node arrays of a single-block domain on its device, built once, and the ``fg_point_grid`` record of a call, filled from
    the block's live tensors (the boundary tensors of a face can be rebound between steps)."""

    def __init__(self, domain):
        require_single_block(domain, "PointGrid")
        self.domain = domain
        blk, s = domain.getBlock(0), domain.solver
        self.dims, self.dtype, self.device = int(domain.dims), domain.dtype, s.velocity.device
        self.np_dtype = np.float64 if self.dtype == torch.float64 else np.float32
        self.periodic = tuple(not blk.isFixed(2 * a) for a in range(self.dims))
        arrays = node_arrays(blk.edges, self.periodic, self.np_dtype)
        self.nodes_host = [a[0] for a in arrays]
        self.lo = np.array([a[1] for a in arrays], self.np_dtype)
        self.len = np.array([a[2] for a in arrays], self.np_dtype)
        self.nodes = [torch.from_numpy(n.copy()).to(self.device) for n in self.nodes_host]
        self.len_dev = torch.from_numpy(self.len.copy()).to(self.device)
        self.lib = F.library(self.dtype)

    def inside(self, positions: np.ndarray) -> bool:
        """Whether every host position ``[..., d]``, rounded to the dtype of the fields, lies in the closed box."""
        p = np.asarray(positions, np.float64).astype(self.np_dtype).astype(np.float64)
        lo = np.array([self.lo[a] if self.periodic[a] else self.nodes_host[a][0] for a in range(self.dims)], np.float64)
        hi = np.array([np.float64(self.lo[a]) + np.float64(self.len[a]) if self.periodic[a] else self.nodes_host[a][-1] for a in range(self.dims)])
        return bool(np.all((p >= lo) & (p <= hi)))

    def record(self):
        """``(fg_point_grid, tensors to keep alive)`` for the fields as they are bound now."""
        s = self.domain.solver
        keep = []

        def env_major(t, what):
            if not t[0].is_contiguous():
                t = t.contiguous()
            keep.append(t)
            per_env = int(t[0].numel())
            return t.data_ptr(), (int(t.stride(0)) if t.shape[0] > 1 else per_env)

        g = (L.FgPointGridF64 if self.dtype == torch.float64 else L.FgPointGrid)()
        g.dims, g.batch, g.nx, g.ny, g.nz = self.dims, int(s.B), int(s.nx), int(s.ny), (int(s.nz) if self.dims == 3 else 1)
        for a in range(self.dims):
            g.periodic[a] = int(self.periodic[a])
            g.nodes[a] = self.nodes[a].data_ptr()
            g.lo[a], g.len[a] = float(self.lo[a]), float(self.len[a])
        g.velocity, g.velocity_stride = env_major(s.velocity, "velocity")
        for a in range(self.dims):
            if not self.periodic[a]:
                for f in (2 * a, 2 * a + 1):
                    g.bvel[f], g.bvel_stride[f] = env_major(s.bvel[f], "boundary velocity")
        return g, keep

    def extra_tables(self, names: Sequence[str]):
        """The pointer and stride tables of the fields ``names`` (``p``, ``T``) and the tensors behind them."""
        s = self.domain.solver
        src = {"p": s.pressure, "T": s.scalar}
        ptrs, strides, keep = [], [], []
        for name in names:
            t = src[name]
            if t is None:
                raise ValueError(f"field {name!r}: the domain has no such field")
            if not t[0].is_contiguous():
                t = t.contiguous()
            keep.append(t)
            ptrs.append(t.data_ptr())                  # channel 0 of [B, C, (Z,) Y, X]
            strides.append(int(t.stride(0)) if t.shape[0] > 1 else int(t[0].numel()))
        n = len(names)
        return (ctypes.c_void_p * max(n, 1))(*ptrs), (ctypes.c_int64 * max(n, 1))(*strides), keep

    def sample(self, points: torch.Tensor, fields: Optional[Sequence[str]] = None) -> torch.Tensor:
        """Values of ``fields`` at ``points`` (``[P, d]``: one point set for all envs, or ``[B, P, d]``), ``[B, P, K]``."""
        dom, d = self.domain, self.dims
        extras, pick = requested_fields(fields, default_fields(dom), FIELD_NAMES, d)
        if not isinstance(points, torch.Tensor):
            points = torch.from_numpy(np.ascontiguousarray(np.asarray(points, np.float64)))
        B = int(dom.solver.B)
        if points.dim() not in (2, 3) or points.shape[-1] != d or (points.dim() == 3 and points.shape[0] != B) or points.shape[-2] < 1:
            raise ValueError(f"points must be [P, {d}] or [{B}, P, {d}] with P >= 1, got {tuple(points.shape)}")
        pts = points.to(self.device, self.dtype).contiguous()
        P = int(pts.shape[-2])
        out = torch.empty(B, P, d + len(extras), dtype=self.dtype, device=self.device)
        g, keep = self.record()
        eptr, estride, ekeep = self.extra_tables(extras)
        with torch.cuda.device(self.device):
            L.check(self.lib.fg_point_sample(ctypes.byref(g), eptr, estride, len(extras), F.ptr(pts), P * d if pts.dim() == 3 else 0, P,
                                             F.ptr(out), F.stream_ptr(self.device)), lib=self.lib)
        return pick(out)


def sample_points(domain, points, fields: Optional[Sequence[str]] = None) -> torch.Tensor:
    """``fields`` (default ``u, v(, w), p(, T)``) of the single-block ``domain`` at the physical positions ``points`` (``[P, d]`` for
    all envs or ``[B, P, d]``), on the GPU: ``[B, P, len(fields)]``."""
    return PointGrid(domain).sample(points, fields)


def seed_positions(seed: int, batch: int, n: int, lo, length) -> np.ndarray:
    """The seeded initial positions ``[batch, n, d]`` in fp64.  Draw order: env ``b`` has its own generator
    ``np.random.default_rng([seed, b])`` and takes ONE draw from it, ``rng.random((n, d))`` -- uniform numbers in ``[0, 1)`` in row-major
    order, i.e. tracer 0's x, y(, z), then tracer 1's, ...; position = ``lo + r * length`` per axis.  An env's seeds therefore do
    not depend on the batch size."""
    lo, length = np.asarray(lo, np.float64), np.asarray(length, np.float64)
    return np.stack([lo + np.random.default_rng([int(seed), b]).random((int(n), len(lo))) * length for b in range(int(batch))])


def respawn_mask(faces, dims: int, periodic) -> int:
    """The bit mask of ``respawn_faces`` (face names or indices); ``ValueError`` for a face the grid does not have or a periodic one."""
    mask = 0
    for face in faces:
        f = face_index(face)
        if not 0 <= f < 2 * dims:
            raise ValueError(f"respawn_faces: face {face!r} does not exist on a {dims}-D grid")
        if periodic[f >> 1]:
            raise ValueError(f"respawn_faces: face {face!r} is periodic; only FIXED faces respawn")
        mask |= 1 << f
    return mask


class CloudBase:
    """What ``TracerCloud`` and ``mb_tracers.MeshTracerCloud`` share.  A cloud names its state tensors in ``_STATE``, the (live, seed)
    attribute pairs a reseed copies in ``_SEEDED`` and the integer settings that travel in its state beside ``substeps`` in
    ``_SCALARS``; it has ``age``, ``wraps`` and ``lost`` among its tensors and an ``unwrapped()``."""
    _STATE: tuple = ()
    _SEEDED: tuple = ()
    _SCALARS: tuple = ()

    def __init__(self, n: int, seed: Optional[int], positions, substeps: int):
        name = type(self).__name__
        if (seed is None) == (positions is None):
            raise ValueError(f"{name}: give exactly one of seed and positions")
        if int(n) < 1:
            raise ValueError(f"{name}: n must be at least 1, got {n}")
        if int(substeps) < 1:
            raise ValueError(f"{name}: substeps must be at least 1, got {substeps}")
        self.n, self.substeps, self.seed = int(n), int(substeps), seed

    @property
    def batch(self) -> int:
        return int(self.positions.shape[0])

    def displacement(self) -> torch.Tensor:
        """The unwrapped path relative to the seed position."""
        return self.unwrapped() - self.seed_positions

    def reseed(self, envs=None) -> None:
        """Return the tracers of the envs ``envs`` (indices or a bool mask; None: all) to their seeds with age, wraps and the lost count
        zero; the other envs keep their bits."""
        cleared = (self.age, self.wraps, self.lost)
        if envs is None:
            for live, seed in self._SEEDED:
                getattr(self, live).copy_(getattr(self, seed))
            for t in cleared:
                t.zero_()
            return
        idx = torch.as_tensor(normalize_envs(envs, self.batch), dtype=torch.int64, device=self.positions.device)
        for live, seed in self._SEEDED:
            getattr(self, live).index_copy_(0, idx, getattr(self, seed).index_select(0, idx))
        for t in cleared:
            t.index_fill_(0, idx, 0)

    def state_dict(self) -> dict:
        return {**{k: getattr(self, k).clone() for k in self._STATE}, **{k: getattr(self, k) for k in ("substeps",) + self._SCALARS}}

    def load_state_dict(self, state: dict) -> None:
        for k in self._STATE:
            if tuple(state[k].shape) != tuple(getattr(self, k).shape):
                raise ValueError(f"{type(self).__name__}.load_state_dict: {k} has shape {tuple(state[k].shape)}, this cloud "
                                 f"{tuple(getattr(self, k).shape)}")
        for k in self._STATE:
            getattr(self, k).copy_(state[k])
        for k in ("substeps",) + self._SCALARS:
            setattr(self, k, int(state[k]))


class TracerCloud(CloudBase):
    """``n`` passive tracers in every env of a single-block ``domain``.

    ``seed``: initial positions uniform in the domain box, drawn on the host per env (``seed_positions`` records the exact draw
    order), so an env's seeds do not depend on the batch size.  ``positions``: ``[N, d]`` (every env the same) or ``[B, N, d]``;
    a position outside the box is a ``ValueError``.  ``respawn_faces``: FIXED faces (names or indices) beyond which a tracer returns
    to its seed position with age 0 (an inflow / outflow pair); beyond any other FIXED face the position is clamped to the face.

    ``positions`` ``[B, N, d]``, ``age`` ``[B, N]``, ``wraps`` ``[B, N, d]`` (int32, signed seam crossings) and ``lost`` ``[B]`` (int32: how often a
    tracer of the env reached a non-finite position and was respawned) live on the GPU."""

    def __init__(self, domain, n: int, seed: Optional[int] = None, positions=None, substeps: int = 4, respawn_faces=()):
        require_single_block(domain, "TracerCloud")
        super().__init__(n, seed, positions, substeps)
        self.grid = g = PointGrid(domain)
        self.respawn_faces = respawn_mask(respawn_faces, g.dims, g.periodic)
        B, d = int(domain.solver.B), g.dims
        if seed is not None:
            host = seed_positions(seed, B, self.n, g.lo.astype(np.float64), g.len.astype(np.float64))
        else:
            host = np.asarray(positions.detach().cpu() if isinstance(positions, torch.Tensor) else positions, np.float64)
            if host.shape not in ((self.n, d), (B, self.n, d)):
                raise ValueError(f"TracerCloud: positions must be [{self.n}, {d}] or [{B}, {self.n}, {d}], got {host.shape}")
            if not g.inside(host):          # (a NaN is outside too)
                raise ValueError("TracerCloud: a position lies outside the domain box")
            host = np.broadcast_to(host, (B, self.n, d))
        self.seed_positions = torch.from_numpy(np.ascontiguousarray(host.astype(g.np_dtype))).to(g.device)
        self.positions = self.seed_positions.clone()
        self.age = torch.zeros(B, self.n, dtype=g.dtype, device=g.device)
        self.wraps = torch.zeros(B, self.n, d, dtype=torch.int32, device=g.device)
        self.lost = torch.zeros(B, dtype=torch.int32, device=g.device)

    _STATE = ("positions", "seed_positions", "age", "wraps", "lost")
    _SEEDED = (("positions", "seed_positions"),)
    _SCALARS = ("respawn_faces",)

    def advect(self, dt: float) -> None:
        """Advance all tracers by ``dt`` in the velocity field as it stands: one launch."""
        g = self.grid
        rec, keep = g.record()
        with torch.cuda.device(g.device):
            L.check(g.lib.fg_tracer_advect(ctypes.byref(rec), float(dt), self.substeps, self.respawn_faces, F.ptr(self.seed_positions),
                                           F.ptr(self.positions), F.ptr(self.age), F.ptr(self.wraps), F.ptr(self.lost), self.n,
                                           F.stream_ptr(g.device)), lib=g.lib)

    def unwrapped(self) -> torch.Tensor:
        """``positions + wraps * length``: the path without the jumps at the periodic seams."""
        return self.positions + self.wraps.to(self.positions.dtype) * self.grid.len_dev

    def sample(self, fields: Optional[Sequence[str]] = None) -> torch.Tensor:
        """Field values at the tracers, ``[B, N, K]``."""
        return self.grid.sample(self.positions, fields)

    def save(self, path) -> None:
        """One ``.npz``: the state arrays, the box (``lo``, ``length``, ``periodic``), ``substeps`` and ``respawn_faces``."""
        g = self.grid
        np.savez(path, **{k: getattr(self, k).cpu().numpy() for k in self._STATE}, lo=g.lo, length=g.len,
                 periodic=np.asarray(g.periodic, np.int32), substeps=np.int32(self.substeps), respawn_faces=np.int32(self.respawn_faces))
