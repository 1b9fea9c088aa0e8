"""Point probes and Lagrangian tracers of a multi-block curvilinear domain on the GPU (``csrc/fg_mb_tracers.hip``; DESIGN.md section
6q): the cylinder and airfoil meshes, where a position becomes a cell only by a walk over the neighbour table and an inverse map.

One interpolant for probes and tracers.  Two block vertices are one *mesh vertex* where a face that two cells share (``neighbors()``)
identifies them; a field has a value at every mesh vertex, a weighted sum over the cells that touch it -- or, for the velocity at
a vertex on a FIXED face, over the boundary slots that touch it and nothing else, so that a point on a wall reads the wall's velocity.
The weights (``vertex_weights``) reproduce affine fields where the stencil allows it.  The value at a point is the multilinear blend of
the ``2^d`` vertex values of the cell that contains it, with the cell's local coordinates ``xi``: continuous across every face, seam
and singular vertex.

``build_point_tables`` is pure NumPy; ``MbPointMesh`` uploads its tables once per domain; ``MeshProbes`` locates points once and
samples them in one launch per call; ``MeshTracerCloud`` moves particles with the flow, crossing connections and periodic faces,
stopping on walls and returning to its seeds at the faces named in ``respawn_slots``.

Not here: inertial particles, interpolation of the velocity in time between sim steps, drawing tracers into ``render_frames``.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np
import torch

from .. import _lib as L
from . import plane_fields as F
from .tracers import CloudBase, requested_fields

FIELD_NAMES = ("u", "v", "w", "p")
MAX_EXTRA, MAX_STENCIL, MAX_SHIFTS = 8, 16, 4
# slack = SLACK_FACTOR * eps(dtype) * max over cells (max |vertex coordinate| / shortest edge): four times the largest ratio of the
# fp32 Newton floor to eps * |x| / edge seen on the test and env meshes, 0.98
SLACK_FACTOR = 4.0
# cell changes a walk may take: a first location from the nearest centre; a walk from a tracer's own cell (MBT_ADVECT_WALK of the kernel)
FIRST_WALK, TRACER_WALK, ACCEPT_RESIDUAL = 256, 64, 1e-9


@dataclass
class MbPointTables:
    dims: int
    n_cells: int
    n_slots: int
    n_vertices: int
    cell_vert: np.ndarray        # [N, 2^d] int32: merged vertex ids (corner k: bit 0 = x, bit 1 = y, bit 2 = z)
    cell_xyz: np.ndarray         # [N, 2^d, d] float64: the corners as the cell's own block stores them
    neighbors: np.ndarray        # [2d, N] int32
    vel_idx: np.ndarray          # [V, Kv] int32 (>= N: boundary slot idx - N)
    vel_w: np.ndarray            # [V, Kv] float64
    cell_idx: np.ndarray         # [V, Kc] int32
    cell_w: np.ndarray           # [V, Kc] float64
    exact: np.ndarray            # [V] bool: the velocity weights solve sum w = 1, sum w d = 0
    cell_exact: np.ndarray       # [V] bool: the same of the scalar weights
    on_fixed: np.ndarray         # [V] bool: the vertex lies on a FIXED face
    face_code: np.ndarray        # [2d, N] uint8: 0, or 1 + 2 s (position -= shifts[s], crossing +1), 2 + 2 s (the reverse)
    shifts: np.ndarray           # [S, d] float64
    mesh_ratio: float            # max over cells (max |vertex coordinate| / shortest edge)
    centres: np.ndarray          # [N, d]
    volumes: np.ndarray          # [N]: |det J| at the cell centre
    bounds: np.ndarray           # [2, d]

    def slack(self, np_dtype) -> float:
        return float(SLACK_FACTOR * np.finfo(np_dtype).eps * self.mesh_ratio)


def _corner_bits(dims: int) -> np.ndarray:
    return np.array([[(k >> a) & 1 for a in range(dims)] for k in range(1 << dims)])


def _face_corners(dims: int, face: int) -> list:
    """The corners of a cell on face ``face`` in the order of the remaining axes' bits."""
    a, side = face >> 1, face & 1
    return [k for k in range(1 << dims) if ((k >> a) & 1) == side]


def _face_matchings(dims: int) -> list:
    """The ways the ``2^(d-1)`` vertices of a face can meet those of the neighbour's face: 2 of an edge, the 8 symmetries of a quad."""
    if dims == 2:
        return [(0, 1), (1, 0)]
    out = []
    for swap in (False, True):
        for f0 in (0, 1):
            for f1 in (0, 1):
                perm = []
                for k in range(4):
                    b0, b1 = k & 1, k >> 1
                    if swap:
                        b0, b1 = b1, b0
                    perm.append((b0 ^ f0) | ((b1 ^ f1) << 1))
                out.append(tuple(perm))
    return out


def vertex_weights(offsets: np.ndarray):
    """Weights of one stencil with offsets ``d_k = x_k - x_v`` (``[K, d]`` or ``[n, K, d]``): ``w = pinv(A) e_1`` of
    ``A = [1 ... 1; d_1 / R ... d_K / R]``, ``R = max |d_k|`` -- the minimum-norm solution of ``sum w = 1, sum w d = 0`` --, accepted where
    ``max |A w - e_1| <= 1e-9``; else ``w_k`` proportional to ``1 / |d_k|``.  Returns ``(w, accepted)``."""
    d = np.asarray(offsets, np.float64)
    single = d.ndim == 2
    if single:
        d = d[None]
    n, K, dims = d.shape
    r = np.linalg.norm(d, axis=2)                                   # [n, K]
    R = r.max(axis=1)
    A = np.concatenate([np.ones((n, 1, K)), (d / R[:, None, None]).transpose(0, 2, 1)], axis=1)     # [n, d + 1, K]
    w = np.linalg.pinv(A)[:, :, 0]                                   # [n, K]
    res = np.einsum("nik,nk->ni", A, w)
    res[:, 0] -= 1.0
    ok = np.abs(res).max(axis=1) <= ACCEPT_RESIDUAL
    inv = 1.0 / r
    w = np.where(ok[:, None], w, inv / inv.sum(axis=1, keepdims=True))
    return (w[0], bool(ok[0])) if single else (w, ok)


def _ell(vertex: np.ndarray, index: np.ndarray, offset: np.ndarray, V: int, what: str):
    """ELL tables ``(idx [V, K], w [V, K], exact [V])`` of the stencil entries ``(vertex, index, offset)``."""
    order = np.lexsort((index, vertex))
    vertex, index, offset = vertex[order], index[order], offset[order]
    count = np.bincount(vertex, minlength=V)
    if count.min() < 1:
        raise ValueError(f"build_point_tables: a vertex without a {what} stencil")
    K = int(count.max())
    if K > MAX_STENCIL:
        raise NotImplementedError(f"build_point_tables: a {what} stencil of {K} entries (more than {MAX_STENCIL})")
    start = np.concatenate([[0], np.cumsum(count)[:-1]])
    idx, w, exact = np.zeros((V, K), np.int32), np.zeros((V, K)), np.zeros(V, bool)
    for k in np.unique(count):
        vs = np.nonzero(count == k)[0]
        rows = start[vs][:, None] + np.arange(k)[None]
        wk, ok = vertex_weights(offset[rows])
        idx[vs, :k], w[vs, :k], exact[vs] = index[rows], wk, ok
    return idx, w, exact


def build_point_tables(block_coords, block_sizes, cell_offsets, neighbors, bcell, bface, dims: int) -> MbPointTables:
    """The host tables of the interpolant and the walk from what ``MBBlock.coords`` / ``size`` / ``cell_offset``,
    ``MultiBlockDomain.neighbors()`` and ``boundary_tables()`` give.  Pure NumPy, fp64."""
    dims = int(dims)
    nbr = np.ascontiguousarray(np.asarray(neighbors, np.int32))
    N, NB, C = int(nbr.shape[1]), int(len(bcell)), 1 << dims
    bits = _corner_bits(dims)
    cell_bv, cell_xyz = np.zeros((N, C), np.int64), np.zeros((N, C, dims))
    edge_pos = np.zeros((N, dims), np.int8)        # per axis: bit 0 the cell is in the first layer of its block, bit 1 in the last
    block_of, voff = np.zeros(N, np.int32), 0
    for b, (coords, size, off) in enumerate(zip(block_coords, block_sizes, cell_offsets)):
        coords = np.asarray(coords, np.float64)
        size3 = tuple(int(s) for s in size) + (1,) * (3 - dims)
        nv = [s + 1 for s in size][:dims]
        grids = np.meshgrid(*[np.arange(s) for s in reversed(size3[:dims])], indexing="ij")[::-1]        # i, j(, k) of [(nz,) ny, nx]
        ijk = [g.reshape(-1) for g in grids]
        n = ijk[0].size
        block_of[off:off + n] = b
        for k in range(C):
            vi = [ijk[a] + bits[k, a] for a in range(dims)]
            flat = vi[dims - 1]
            for a in range(dims - 2, -1, -1):
                flat = flat * nv[a] + vi[a]
            cell_bv[off:off + n, k] = voff + flat
            cell_xyz[off:off + n, k] = np.stack([coords[(a,) + tuple(vi[::-1])] for a in range(dims)], axis=1)
        for a in range(dims):
            edge_pos[off:off + n, a] = (ijk[a] == 0).astype(np.int8) + 2 * (ijk[a] == size3[a] - 1).astype(np.int8)
        voff += int(np.prod(nv))
    lo, hi = cell_xyz.reshape(-1, dims).min(0), cell_xyz.reshape(-1, dims).max(0)
    extent = float((hi - lo).max())

    # mesh vertices: union-find over the faces two cells share across a block edge (inside a block the vertex array is shared already)
    parent = np.arange(voff)

    def find(i):
        root = i
        while parent[root] != root:
            root = parent[root]
        while parent[i] != root:
            parent[i], i = root, parent[i]
        return root

    face_code = np.zeros((2 * dims, N), np.uint8)
    shifts: list = []
    matchings = _face_matchings(dims)
    tol = 1e-5 * extent
    for f in range(2 * dims):
        a, side = f >> 1, f & 1
        at_edge = (edge_pos[:, a] >> side) & 1
        mine = _face_corners(dims, f)
        for c in np.nonzero((at_edge == 1) & (nbr[f] >= 0))[0]:
            o = int(nbr[f, c])
            # the face of the neighbour that leads back: the opposite one of a periodic axis, else the first block-edge face that does
            back = -1
            if block_of[o] == block_of[c] and nbr[f ^ 1, o] == c and (edge_pos[o, a] >> (side ^ 1)) & 1:
                back = f ^ 1
            else:
                for g in range(2 * dims):
                    if nbr[g, o] == c and (edge_pos[o, g >> 1] >> (g & 1)) & 1:
                        back = g
                        break
            if back < 0:
                raise ValueError(f"build_point_tables: cell {o} has no face that leads back to cell {c}")
            theirs = _face_corners(dims, back)
            xa, xb = cell_xyz[c, mine], cell_xyz[o, theirs]
            best, best_spread, best_diff = None, np.inf, None
            for perm in matchings:
                diff = xa - xb[list(perm)]
                spread = np.abs(diff - diff.mean(0)).max()
                if spread < best_spread:
                    best, best_spread, best_diff = perm, spread, diff.mean(0)
            if best_spread > tol:
                raise ValueError(f"build_point_tables: face {f} of cell {c} and face {back} of cell {o} do not differ by one constant vector")
            for k, kk in zip(mine, best):
                ra, rb = find(cell_bv[c, k]), find(cell_bv[o, theirs[kk]])
                if ra != rb:
                    parent[max(ra, rb)] = min(ra, rb)
            if np.abs(best_diff).max() > tol:       # a periodic face: in the neighbour's image the position is p - diff
                code = 0
                for s, vec in enumerate(shifts):
                    if np.abs(vec - best_diff).max() <= tol:
                        code = 1 + 2 * s
                    elif np.abs(vec + best_diff).max() <= tol:
                        code = 2 + 2 * s
                if code == 0:
                    if block_of[o] != block_of[c] or back != (f ^ 1):
                        raise ValueError(f"build_point_tables: the connection of cells {c} and {o} shifts positions by {best_diff}")
                    shifts.append(best_diff if side else -best_diff)
                    code = (1 if side else 2) + 2 * (len(shifts) - 1)
                face_code[f, c] = code
    if len(shifts) > MAX_SHIFTS:
        raise NotImplementedError(f"build_point_tables: {len(shifts)} periodic shift vectors (more than {MAX_SHIFTS})")
    while True:
        nxt = parent[parent]
        if np.array_equal(nxt, parent):
            break
        parent = nxt
    roots, merged = np.unique(parent, return_inverse=True)
    V = int(len(roots))
    cell_vert = merged[cell_bv].astype(np.int32)

    # stencil entries: every (cell, corner) for the cells that touch a vertex; every (FIXED face, corner) for the slots that do
    centres = cell_xyz.mean(axis=1)
    cv, cidx = cell_vert.reshape(-1).astype(np.int64), np.repeat(np.arange(N, dtype=np.int64), C)
    coff = (centres[:, None, :] - cell_xyz).reshape(-1, dims)
    bcell, bface = np.asarray(bcell, np.int64), np.asarray(bface, np.int64)
    sv, sidx, soff = [], [], []
    for f in range(2 * dims):
        slots = np.nonzero(bface == f)[0]
        if not len(slots):
            continue
        cells = bcell[slots]
        if not np.array_equal(nbr[f, cells], (-1 - slots).astype(np.int32)):
            raise ValueError("build_point_tables: the boundary tables and the neighbour table disagree")
        corners = _face_corners(dims, f)
        fc = cell_xyz[cells][:, corners].mean(axis=1)                 # [n, d] face centres
        for k in corners:
            sv.append(cell_vert[cells, k].astype(np.int64)); sidx.append(N + slots); soff.append(fc - cell_xyz[cells, k])
    if int((nbr < 0).sum()) != NB:
        raise ValueError("build_point_tables: the neighbour table names another number of boundary slots than the boundary tables")
    on_fixed = np.zeros(V, bool)
    if sv:
        sv, sidx, soff = np.concatenate(sv), np.concatenate(sidx), np.concatenate(soff)
        on_fixed[sv] = True
        free = ~on_fixed[cv]
        vv, vi, vo = np.concatenate([cv[free], sv]), np.concatenate([cidx[free], sidx]), np.concatenate([coff[free], soff])
    else:
        vv, vi, vo = cv, cidx, coff
    vel_idx, vel_w, exact = _ell(vv, vi, vo, V, "velocity")
    cell_idx, cell_w, cell_exact = _ell(cv, cidx, coff, V, "cell")

    # the resolution of xi: |x| / shortest edge per cell; the volume |det J| at the centre
    shortest = np.full(N, np.inf)
    for k in range(C):
        for a in range(dims):
            if not bits[k, a]:
                shortest = np.minimum(shortest, np.linalg.norm(cell_xyz[:, k | (1 << a)] - cell_xyz[:, k], axis=1))
    if not shortest.min() > 0:
        raise ValueError("build_point_tables: a cell edge of length zero")
    ratio = float((np.abs(cell_xyz).reshape(N, -1).max(axis=1) / shortest).max())
    J = np.zeros((N, dims, dims))
    for a in range(dims):
        hi_k = [k for k in range(C) if bits[k, a]]
        lo_k = [k for k in range(C) if not bits[k, a]]
        J[:, :, a] = cell_xyz[:, hi_k].mean(axis=1) - cell_xyz[:, lo_k].mean(axis=1)
    return MbPointTables(dims=dims, n_cells=N, n_slots=NB, n_vertices=V, cell_vert=cell_vert, cell_xyz=cell_xyz, neighbors=nbr,
                         vel_idx=vel_idx, vel_w=vel_w, cell_idx=cell_idx, cell_w=cell_w, exact=exact, cell_exact=cell_exact,
                         on_fixed=on_fixed, face_code=face_code, shifts=np.array(shifts, np.float64).reshape(-1, dims), mesh_ratio=ratio,
                         centres=centres, volumes=np.abs(np.linalg.det(J)), bounds=np.stack([lo, hi]))


def domain_point_tables(domain) -> MbPointTables:
    """``build_point_tables`` of a prepared ``MultiBlockDomain``."""
    if not getattr(domain, "prepared", False):
        raise RuntimeError("PrepareSolve() the domain first")
    bcell, bface, _ = domain.boundary_tables()
    return build_point_tables([b.coords for b in domain.blocks], [b.size for b in domain.blocks], [b.cell_offset for b in domain.blocks],
                              domain.neighbors(), bcell, bface, domain.dims)


def nearest_cells(centres: np.ndarray, points: np.ndarray) -> np.ndarray:
    """The index of the nearest cell centre of every point (``scipy.spatial.cKDTree`` if importable, else chunked brute force); a
    non-finite point gets cell 0."""
    pts = np.asarray(points, np.float64).reshape(-1, centres.shape[1])
    ok = np.isfinite(pts).all(axis=1)
    out = np.zeros(len(pts), np.int32)
    if ok.any():
        try:
            from scipy.spatial import cKDTree
            out[ok] = cKDTree(centres).query(pts[ok])[1]
        except ImportError:
            good = pts[ok]
            found = np.zeros(len(good), np.int32)
            for i in range(0, len(good), 1024):
                d2 = ((good[i:i + 1024, None, :] - centres[None]) ** 2).sum(-1)
                found[i:i + 1024] = d2.argmin(axis=1)
            out[ok] = found
    return out.reshape(np.asarray(points).shape[:-1])


def cell_map(corners: np.ndarray, xi: np.ndarray) -> np.ndarray:
    """The bi- / trilinear map of cells with corners ``[..., 2^d, d]`` at ``xi [..., d]`` (x first, then y, then z)."""
    v = np.asarray(corners, np.float64)
    for a in range(xi.shape[-1]):
        v = v[..., 0::2, :] + xi[..., a, None, None] * (v[..., 1::2, :] - v[..., 0::2, :])
    return v[..., 0, :]


def seed_cells_and_xi(seed: int, batch: int, n: int, volumes: np.ndarray, dims: int):
    """The seeded cells ``[batch, n]`` and local coordinates ``[batch, n, d]``.  Draw order: env ``b`` has its own generator
    ``np.random.default_rng([seed, b])`` and takes ONE draw from it, ``rng.random((n, d + 1))``, row-major; column 0 picks the cell with
    probability proportional to its volume (the first cell whose cumulative volume fraction exceeds it), columns 1.. are ``xi``.  An
    env's seeds do not depend on the batch size, and every seed lies in a cell."""
    cum = np.cumsum(volumes) / volumes.sum()
    cells, xi = np.zeros((batch, n), np.int32), np.zeros((batch, n, dims))
    for b in range(int(batch)):
        r = np.random.default_rng([int(seed), b]).random((int(n), dims + 1))
        cells[b] = np.minimum(np.searchsorted(cum, r[:, 0], side="right"), len(cum) - 1)
        xi[b] = r[:, 1:]
    return cells, xi


class MbPointMesh:
    """The tables of a prepared ``MultiBlockDomain`` on its device, in its dtype, built once and shared by all envs of the batch; the
    ``fg_mb_point_mesh`` record of a call is filled from the domain's live tensors."""

    def __init__(self, domain):
        from .multiblock import MultiBlockDomain

        if not isinstance(domain, MultiBlockDomain):
            raise NotImplementedError("MbPointMesh needs a multi-block domain (cylinder, airfoil envs); single-block domains have "
                                      "sample_points and TracerCloud")
        self.domain = domain
        self.tables = t = domain_point_tables(domain)
        self.dims, self.dtype, self.device = t.dims, domain.dtype, domain.velocity.device
        self.np_dtype = np.float64 if self.dtype == torch.float64 else np.float32
        self.slack = t.slack(self.np_dtype)
        if not 0.0 < self.slack < 0.25:
            raise NotImplementedError(f"MbPointMesh: positions of {self.np_dtype.__name__} resolve the cells' local coordinates to "
                                      f"{self.slack:.3g} only")
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a.astype(dt))).to(self.device)
        self.cell_vert, self.cell_xyz = up(t.cell_vert, np.int32), up(t.cell_xyz, self.np_dtype)
        self.neighbors, self.face_code = up(t.neighbors, np.int32), up(t.face_code, np.uint8)
        self.vel_idx, self.vel_w = up(t.vel_idx, np.int32), up(t.vel_w, self.np_dtype)
        self.cell_idx, self.cell_w = up(t.cell_idx, np.int32), up(t.cell_w, self.np_dtype)
        self.shifts_host = t.shifts.astype(self.np_dtype)
        self.shifts = up(t.shifts, self.np_dtype)
        self.respawn_slots = torch.zeros(max(t.n_slots, 1), dtype=torch.uint8, device=self.device)
        self.lib = F.library(self.dtype)

    def record(self):
        """``(fg_mb_point_mesh, tensors to keep alive)`` for the fields as they are bound now."""
        dom, t = self.domain, self.tables
        vel, bvel = dom.velocity, dom.boundary_velocity
        if not vel.is_contiguous() or not bvel.is_contiguous():
            raise ValueError("MbPointMesh: the domain's velocity and boundary velocity must be contiguous")
        m = (L.FgMbPointMeshF64 if self.dtype == torch.float64 else L.FgMbPointMesh)()
        m.dims, m.batch, m.n_cells, m.n_slots, m.n_vertices = t.dims, int(dom.batch), t.n_cells, t.n_slots, t.n_vertices
        m.kv, m.kc, m.n_shifts = int(t.vel_idx.shape[1]), int(t.cell_idx.shape[1]), int(len(t.shifts))
        for name in ("cell_vert", "cell_xyz", "neighbors", "face_code", "vel_idx", "vel_w", "cell_idx", "cell_w"):
            setattr(m, name, getattr(self, name).data_ptr())
        m.slack = self.slack
        for s, vec in enumerate(self.shifts_host):
            for a in range(t.dims):
                m.shifts[3 * s + a] = float(vec[a])
        m.velocity, m.velocity_stride = vel.data_ptr(), int(vel.shape[1] * vel.shape[2])
        m.bvel, m.bvel_stride, m.bvel_comp_stride = bvel.data_ptr(), int(bvel.shape[1] * bvel.shape[2]), int(bvel.shape[2])
        return m, [vel, bvel]

    def locate(self, points: torch.Tensor, start_cell: torch.Tensor, max_walk: int = FIRST_WALK):
        """``(cell [B, P] int32, xi [B, P, d], status [B, P] int32)`` of ``points`` (``[P, d]`` with ``start_cell [P]``, or ``[B, P, d]``
        with ``[B, P]``) on the device."""
        B, d = int(self.domain.batch), self.dims
        P = int(points.shape[-2])
        cell = torch.empty(B, P, dtype=torch.int32, device=self.device)
        xi = torch.empty(B, P, d, dtype=self.dtype, device=self.device)
        status = torch.empty(B, P, dtype=torch.int32, device=self.device)
        m, keep = self.record()
        with torch.cuda.device(self.device):
            L.check(self.lib.fg_mb_point_locate(ctypes.byref(m), F.ptr(points), P * d if points.dim() == 3 else 0, P, F.ptr(start_cell),
                                                int(max_walk), F.ptr(cell), F.ptr(xi), F.ptr(status), F.stream_ptr(self.device)), lib=self.lib)
        return cell, xi, status

    def locate_host(self, points, what: str):
        """Host points ``[P, d]`` or ``[B, P, d]`` -> ``(device points, cell, xi, status)``: nearest-centre start cells, then the walk."""
        B, d = int(self.domain.batch), self.dims
        host = np.asarray(points.detach().cpu() if isinstance(points, torch.Tensor) else points, np.float64)
        if host.ndim not in (2, 3) or host.shape[-1] != d or (host.ndim == 3 and host.shape[0] != B) or host.shape[-2] < 1:
            raise ValueError(f"{what}: points must be [P, {d}] or [{B}, P, {d}] with P >= 1, got {host.shape}")
        rounded = host.astype(self.np_dtype)
        start = torch.from_numpy(np.ascontiguousarray(nearest_cells(self.tables.centres, rounded.astype(np.float64)))).to(self.device)
        pts = torch.from_numpy(np.ascontiguousarray(rounded)).to(self.device)
        return (pts,) + self.locate(pts, start)

    def sample(self, cell: torch.Tensor, xi: torch.Tensor, fields: Optional[Sequence[str]] = None) -> torch.Tensor:
        """``fields`` (default ``u, v(, w), p``) at the located points ``cell [B, P]`` (or ``[P]``), ``xi [..., P, d]``: ``[B, P, K]``,
        one launch."""
        dom, d = self.domain, self.dims
        extras, pick = requested_fields(fields, ("u", "v") + (("w",) if d == 3 else ()) + ("p",), FIELD_NAMES, d)
        B, P = int(dom.batch), int(cell.shape[-1])
        out = torch.empty(B, P, d + len(extras), dtype=self.dtype, device=self.device)
        m, keep = self.record()
        eptr = estride = None                                        # (no table where no cell-only field is asked for)
        if extras:
            eptr, estride = (ctypes.c_void_p * 1)(dom.pressure.data_ptr()), (ctypes.c_int64 * 1)(int(dom.pressure.shape[1]))
        with torch.cuda.device(self.device):
            L.check(self.lib.fg_mb_point_sample(ctypes.byref(m), eptr, estride, len(extras), F.ptr(cell), F.ptr(xi), P if cell.dim() == 2 else 0,
                                                P, F.ptr(out), F.stream_ptr(self.device)), lib=self.lib)
        return pick(out)


def _mesh_of(domain_or_mesh) -> MbPointMesh:
    return domain_or_mesh if isinstance(domain_or_mesh, MbPointMesh) else MbPointMesh(domain_or_mesh)


class MeshProbes:
    """Point probes of a multi-block ``domain`` (or its ``MbPointMesh``) at the physical positions ``points`` (``[P, d]`` for every
    env, or ``[B, P, d]``), located once.  ``status`` ``[B, P]``: 0 found, 1 outside the fluid (the probe sits on the FIXED face the
    walk stopped at), 2 not found.  ``strict=True`` raises ``ValueError`` for the first point with a non-zero status; ``strict=False``
    keeps the clamped location.  ``sample(fields)`` is one launch and returns nothing to the host."""

    def __init__(self, domain, points, strict: bool = True):
        self.mesh = _mesh_of(domain)
        self.points, self.cell, self.xi, self.status = self.mesh.locate_host(points, "MeshProbes")
        if strict:
            st = self.status.cpu().numpy()
            if st.any():
                b, p = np.argwhere(st != 0)[0]
                pos = self.points.cpu().numpy().reshape(-1, self.points.shape[-2], self.mesh.dims)[b if self.points.dim() == 3 else 0, p]
                raise ValueError(f"MeshProbes: point {int(p)} of env {int(b)} at {pos.tolist()} is "
                                 f"{'outside the fluid' if st[b, p] == 1 else 'not found'} (status {int(st[b, p])}); strict=False keeps "
                                 "the nearest location on the boundary")

    def sample(self, fields: Optional[Sequence[str]] = None) -> torch.Tensor:
        return self.mesh.sample(self.cell, self.xi, fields)


class MeshTracerCloud(CloudBase):
    """``n`` passive tracers in every env of a multi-block ``domain`` (or its ``MbPointMesh``).

    ``seed``: per env a cell drawn with probability proportional to its volume and a uniform ``xi`` mapped through it
    (``seed_cells_and_xi`` records the draw order): every seed lies in the fluid, and an env's seeds do not depend on the batch size.
    ``positions``: ``[N, d]`` or ``[B, N, d]``, each located by a walk; a position outside the fluid is a ``ValueError``.
    ``respawn_slots``: boundary slots (indices, or a bool / uint8 ``[NB]`` mask) at which a tracer returns to its seed with age 0 (inflow
    and outflow faces); at any other FIXED face it stops on the face.

    ``positions`` ``[B, N, d]``, ``cell`` ``[B, N]`` (int32), ``age`` ``[B, N]``, ``wraps`` ``[B, N, S]`` (int32: signed crossings per periodic
    shift vector) and ``lost`` ``[B]`` (int32: how often a tracer of the env reached a non-finite position or exhausted its walk and was
    respawned) live on the GPU."""

    def __init__(self, domain, n: int, seed: Optional[int] = None, positions=None, substeps: int = 4, respawn_slots=None):
        super().__init__(n, seed, positions, substeps)
        self.mesh = m = _mesh_of(domain)
        t = m.tables
        B, d = int(m.domain.batch), m.dims
        self.respawn_slots = m.respawn_slots.clone()
        if respawn_slots is not None:
            r = np.asarray(respawn_slots.cpu() if isinstance(respawn_slots, torch.Tensor) else respawn_slots)
            mask = np.zeros(max(t.n_slots, 1), np.uint8)
            if r.dtype == bool or (r.dtype == np.uint8 and r.shape == (t.n_slots,)):
                mask[:t.n_slots] = r != 0
            else:
                if r.size and (r.min() < 0 or r.max() >= t.n_slots):
                    raise ValueError(f"MeshTracerCloud: respawn_slots names a slot outside 0..{t.n_slots - 1}")
                mask[r.astype(np.int64)] = 1
            self.respawn_slots = torch.from_numpy(mask).to(m.device)
        if seed is not None:
            cells, xi = seed_cells_and_xi(seed, B, self.n, t.volumes, d)
            host = cell_map(t.cell_xyz[cells], xi).astype(m.np_dtype)
            self.seed_positions = torch.from_numpy(np.ascontiguousarray(host)).to(m.device)
            self.seed_cell = torch.from_numpy(cells).to(m.device)
        else:
            host = np.asarray(positions.detach().cpu() if isinstance(positions, torch.Tensor) else positions, np.float64)
            if host.shape not in ((self.n, d), (B, self.n, d)):
                raise ValueError(f"MeshTracerCloud: positions must be [{self.n}, {d}] or [{B}, {self.n}, {d}], got {host.shape}")
            pts, cell, _, status = m.locate_host(host, "MeshTracerCloud")
            if bool((status != 0).any()):
                raise ValueError("MeshTracerCloud: a position lies outside the fluid")
            self.seed_positions = pts.expand(B, self.n, d).contiguous()
            self.seed_cell = cell.contiguous()
        self.positions = self.seed_positions.clone()
        self.cell = self.seed_cell.clone()
        self.age = torch.zeros(B, self.n, dtype=m.dtype, device=m.device)
        self.wraps = torch.zeros(B, self.n, len(t.shifts), dtype=torch.int32, device=m.device)
        self.lost = torch.zeros(B, dtype=torch.int32, device=m.device)

    _STATE = ("positions", "seed_positions", "cell", "seed_cell", "age", "wraps", "lost", "respawn_slots")
    _SEEDED = (("positions", "seed_positions"), ("cell", "seed_cell"))

    def advect(self, dt: float) -> None:
        """Advance all tracers by ``dt`` in the velocity field as it stands: one launch."""
        m = self.mesh
        rec, keep = m.record()
        with torch.cuda.device(m.device):
            L.check(m.lib.fg_mb_tracer_advect(ctypes.byref(rec), float(dt), self.substeps, F.ptr(self.respawn_slots), F.ptr(self.seed_positions),
                                              F.ptr(self.seed_cell), F.ptr(self.positions), F.ptr(self.cell), F.ptr(self.age),
                                              F.ptr(self.wraps) if self.wraps.numel() else None, F.ptr(self.lost), self.n,
                                              F.stream_ptr(m.device)), lib=m.lib)

    def unwrapped(self) -> torch.Tensor:
        """``positions + wraps @ shifts``: the path without the jumps at the periodic faces."""
        if not self.wraps.shape[-1]:
            return self.positions.clone()
        return self.positions + self.wraps.to(self.positions.dtype) @ self.mesh.shifts

    def sample(self, fields: Optional[Sequence[str]] = None) -> torch.Tensor:
        """Field values at the tracers, ``[B, N, K]``: the tracers' cells as starts of a walk, then the gather."""
        cell, xi, _ = self.mesh.locate(self.positions, self.cell, max_walk=TRACER_WALK)
        return self.mesh.sample(cell, xi, fields)

    def save(self, path) -> None:
        """One ``.npz``: the state arrays, the periodic ``shifts``, the mesh ``bounds`` and ``substeps``."""
        t = self.mesh.tables
        np.savez(path, **{k: getattr(self, k).cpu().numpy() for k in self._STATE}, shifts=t.shifts, bounds=t.bounds,
                 substeps=np.int32(self.substeps))
