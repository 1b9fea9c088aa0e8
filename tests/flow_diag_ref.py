"""The checker of the velocity-gradient diagnostics (``fg_flow_diagnostic`` / ``fg_mb_flow_diagnostic``, csrc/fg_flowdiag.hip):
NumPy, fp64 arithmetic, no GPU.

* the gradient ``g[i][j] = d u_i / d x_j`` of ``getBlockDataGradient`` (PISO_multiblock_cuda_kernel.cu:2997-3040) -- single-block:
  ``oracle.piso_oracle.velocity_gradient``; multi-block: restated here over ``oracle.mb_oracle.Domain`` (``cells``,
  ``resolve_neighbor``, ``is_empty``, ``bound_value``, ``Tcell``, ``gidx``), never over the library's tables -- each with its
  magnitude companion ``A`` (the same sums with every term replaced by its absolute value), the scale of the rounding bound;
* the derived kinds evaluated in doubles from a given gradient, with the scale of their bound;
* the bounds themselves (``check_gradient``, ``check_derived``), in units of the machine epsilon of the build under test;
* the analytic case: a rigid rotation ``u = Omega x x + c`` on a uniform single-block grid and on a two-block affine (sheared)
  mesh, all coordinates and field values dyadic, so that the fp32 library holds them exactly.

Inputs are the exact values the GPU holds (for the fp32 library: fp32 values promoted to doubles).
"""
from __future__ import annotations

import numpy as np

from oracle import mb_oracle as mbo
from oracle import piso_oracle as O
from tests.helpers import Case
from tests.helpers_mb import Spec

GRADIENT, VORTICITY, VORTICITY_MAGNITUDE, Q, STRAIN_NORM = range(5)
KINDS = (GRADIENT, VORTICITY, VORTICITY_MAGNITUDE, Q, STRAIN_NORM)


def channels(dims: int, kind: int) -> int:
    return dims * dims if kind == GRADIENT else (3 if (kind == VORTICITY and dims == 3) else 1)


# ------------------------------------------------------------------------------------------------ the gradient
def single_block_gradient(dom: O.Domain):
    """``(g, A)``, both ``[d, d, *cells]``: ``g`` is ``velocity_gradient`` of the oracle, ``A[i][a] = (|hi| + |lo|) / dist / h_a``."""
    g = O.velocity_gradient(dom)
    grid, d = dom.grid, dom.dims
    u = np.abs(dom.velocity.reshape((d,) + grid.shape))
    A = np.zeros_like(g)
    for a in range(d):
        mag = np.zeros_like(u)
        dist = np.full(grid.shape, 2.0)
        for up in (0, 1):
            f = 2 * a + up
            val = O._nbr(u, a, 1 if up else -1)
            if dom.is_fixed(f):
                at = O._at_bound(grid, f)
                val = np.where(at, O._slab_to_cells(grid, f, np.abs(dom.bvel(f))), val)
                dist = dist - 0.5 * at
            mag = mag + val
        A[:, a] = mag / dist * np.abs(grid.Minv[..., a, a])
    return g, A


def _exact_inverse(M: np.ndarray) -> np.ndarray:
    """The inverse of one d x d matrix of doubles in rational arithmetic (adjugate / determinant), rounded once."""
    from fractions import Fraction

    d = M.shape[0]
    m = [[Fraction(float(M[i, j])) for j in range(d)] for i in range(d)]
    if d == 2:
        adj = [[m[1][1], -m[0][1]], [-m[1][0], m[0][0]]]
        det = m[0][0] * m[1][1] - m[0][1] * m[1][0]
    else:
        cof = lambda i, j: m[(i + 1) % 3][(j + 1) % 3] * m[(i + 2) % 3][(j + 2) % 3] - m[(i + 1) % 3][(j + 2) % 3] * m[(i + 2) % 3][(j + 1) % 3]
        adj = [[cof(j, i) for j in range(3)] for i in range(3)]
        det = sum(m[0][j] * cof(0, j) for j in range(3))
    return np.array([[float(adj[i][j] / det) for j in range(d)] for i in range(d)])


def cell_metrics(dom: mbo.Domain):
    """Per block the cells' ``Minv`` (array layout of ``Block.Minv``) with every ENTRY rounded once.  ``Tcell`` hands out
    ``np.linalg.inv`` of the cell's ``M``: accurate in norm, but on stretched, skewed cells its entries are off by up to 920 eps64
    (the airfoil mesh at ``div = 4``; the library's adjugate is within 0.87 eps64 of the exact inverse there), where the bound of
    ``check_gradient`` counts ONE rounding per metric entry -- with the raw ``Tcell`` entries the fp64 library reads 13.6 eps A
    on that mesh against the bound of 8, and at most 2.5 on every other mesh.  So the entries are polished: the exact inverse of the
    oracle's own ``M`` of the cell (``coords_to_transforms`` of the block's coordinates, what ``Tcell`` inverted), asserted to agree
    with ``Tcell`` in norm.  Nothing of the library enters."""
    out = []
    for blk in dom.blocks:
        M = O.coords_to_transforms(blk.coords)[0]
        exact = np.empty_like(blk.Minv)
        for ix in np.ndindex(*blk.Minv.shape[:-2]):
            exact[ix] = _exact_inverse(M[ix])
            assert np.abs(exact[ix] - blk.Minv[ix]).max() <= 1e-9 * np.abs(blk.Minv[ix]).max()
        out.append(exact)
    return out


def multi_block_gradient(dom: mbo.Domain, u: np.ndarray):
    """``(g, A)``, both ``[d, d, N]``, for the velocity ``u [d, N]`` and the boundary values the domain holds:
    ``c[i][a] = (hi - lo) / dist`` with the VALUE across each face (the neighbour cell's ``u_i`` -- no axis mapping, also across a
    rotated connection -- or the prescribed face's velocity, which takes half a cell off ``dist``), ``g = c @ Minv``;
    ``A[i][j] = sum_a (|hi| + |lo|) / dist |Minv[a][j]|``.  ``Minv`` is ``Tcell``'s with its entries polished (``cell_metrics``)."""
    d = dom.d
    u = np.asarray(u, np.float64)
    g = np.zeros((d, d, dom.N))
    A = np.zeros((d, d, dom.N))
    metrics = cell_metrics(dom)
    for b, pos in dom.cells():
        Minv_tcell, _ = dom.Tcell(b, pos)
        Minv = metrics[b][tuple(pos[a] for a in reversed(range(d)))]      # Tcell's entries, each rounded once (cell_metrics)
        assert np.abs(Minv - Minv_tcell).max() <= 1e-9 * np.abs(Minv_tcell).max()
        c, ca = np.zeros((d, d)), np.zeros((d, d))
        for a in range(d):
            vals, prescribed = [], 0
            for face in (2 * a, 2 * a + 1):
                if dom.at_bound(b, pos, face) and dom.is_empty(b, face):
                    vals.append(np.array([dom.bound_value(b, face, pos, q) for q in range(d)], np.float64))
                    prescribed += 1
                else:
                    kind, b2, pos2 = dom.resolve_neighbor(b, pos, face)[:3]
                    assert kind == "cell"
                    vals.append(u[:, dom.gidx(b2, pos2)])
            dist = 2.0 - 0.5 * prescribed
            c[:, a] = (vals[1] - vals[0]) / dist
            ca[:, a] = (np.abs(vals[1]) + np.abs(vals[0])) / dist
        i = dom.gidx(b, pos)
        g[:, :, i] = c @ Minv
        A[:, :, i] = ca @ np.abs(Minv)
    return g, A


# ------------------------------------------------------------------------------------------------ derived kinds, in doubles
def derived(g: np.ndarray, kind: int):
    """``(value [K, ...], scale)`` of a derived kind from the gradient ``g [d, d, ...]``: the formula of the kind in doubles and
    the scale its bound multiplies (``sum |terms|`` per channel for the vorticity, ``0.5 sum g^2`` for Q, ``sqrt(sum g^2)`` for
    the two norms)."""
    g = np.asarray(g, np.float64)
    d = g.shape[0]
    sum_g2 = (g * g).sum(axis=(0, 1))
    pairs = [(1, 0)] if d == 2 else [(2, 1), (0, 2), (1, 0)]
    if kind in (VORTICITY, VORTICITY_MAGNITUDE):
        w = np.stack([g[i, j] - g[j, i] for i, j in pairs])
        if kind == VORTICITY:
            return w, np.stack([np.abs(g[i, j]) + np.abs(g[j, i]) for i, j in pairs])
        return np.sqrt((w * w).sum(axis=0))[None], np.sqrt(sum_g2)[None]
    S = 0.5 * (g + g.swapaxes(0, 1))
    if kind == Q:
        W = 0.5 * (g - g.swapaxes(0, 1))
        return (0.5 * ((W * W).sum(axis=(0, 1)) - (S * S).sum(axis=(0, 1))))[None], (0.5 * sum_g2)[None]
    assert kind == STRAIN_NORM
    return np.sqrt(2.0 * (S * S).sum(axis=(0, 1)))[None], np.sqrt(sum_g2)[None]


# ------------------------------------------------------------------------------------------------ the bounds
def check_gradient(gpu: np.ndarray, g: np.ndarray, A: np.ndarray, eps: float, what=""):
    """``|gpu - ref| <= 8 eps A`` in every cell: one subtraction, one division, d products and d - 1 sums, each rounded to eps / 2,
    and one metric entry stored in the build's precision -- about 3.5 eps A in 3-D; the 8 is a margin of two over that."""
    gpu = np.asarray(gpu, np.float64).reshape(g.shape)
    err = np.abs(gpu - g)
    worst = float((err / np.maximum(A, 1e-300)).max() / eps)
    print(f"{what} gradient: max |gpu - ref| / (eps A) = {worst:.3f} (bound 8)")
    assert np.isfinite(gpu).all() and (err <= 8.0 * eps * A).all(), (what, worst)


def check_derived(kind: int, gpu: np.ndarray, gpu_gradient: np.ndarray, eps: float, what=""):
    """A derived kind against its formula in doubles from the GPU's own gradient: linear kinds ``<= 4 eps sum |terms|``, Q
    ``<= 16 eps 0.5 sum g^2``, the norms relative ``8 eps`` -- absolute ``8 eps sqrt(sum g^2)`` where the norm itself is below
    that, i.e. rounding noise of its terms."""
    ref, scale = derived(gpu_gradient, kind)
    gpu = np.asarray(gpu, np.float64).reshape(ref.shape)
    err = np.abs(gpu - ref)
    if kind == VORTICITY:
        tol = 4.0 * eps * scale
    elif kind == Q:
        tol = 16.0 * eps * scale
    else:
        tol = 8.0 * eps * np.where(np.abs(ref) > 8.0 * eps * scale, np.abs(ref), scale)
    worst = float((err / np.maximum(tol, 1e-300)).max())
    print(f"{what} kind {kind}: max error / bound = {worst:.3f}")
    assert np.isfinite(gpu).all() and (err <= tol).all(), (what, kind, worst)


def assert_not_trivial(g: np.ndarray, u_max: float, h_max: float):
    """A zero field cannot pass: ``max |g| > 1e-2 max |u| / max h``."""
    assert float(np.abs(g).max()) > 1e-2 * u_max / h_max


# ------------------------------------------------------------------------------------------------ inputs
def exact_case(case: Case) -> Case:
    """The case with inputs both libraries and the oracle hold exactly: widths on a 2^-12 lattice (so that the edges' differences
    are the widths again, in doubles), fields and boundary values rounded to fp32."""
    case.widths = [np.maximum(np.round(np.asarray(w, np.float64) * 4096.0), 1.0).astype(np.float32) / np.float32(4096.0) for w in case.widths]
    case.edges = [np.concatenate([[0.0], np.cumsum(w.astype(np.float64))]) for w in case.widths]
    case.velocity = case.velocity.astype(np.float32).astype(np.float64)
    case.bvel = {f: v.astype(np.float32).astype(np.float64) for f, v in case.bvel.items()}
    return case


def rigid_rotation(x: np.ndarray, omega, c) -> np.ndarray:
    """``u = Omega x x + c`` at the points ``x [d, ...]``: ``omega`` a scalar in 2-D (rotation about z), a 3-vector in 3-D."""
    d = x.shape[0]
    c = np.asarray(c, np.float64).reshape((d,) + (1,) * (x.ndim - 1))
    if d == 2:
        return np.stack([-omega * x[1], omega * x[0]]) + c
    w = np.asarray(omega, np.float64)
    return np.stack([w[1] * x[2] - w[2] * x[1], w[2] * x[0] - w[0] * x[2], w[0] * x[1] - w[1] * x[0]]) + c


def rigid_expected(dims: int, omega):
    """``(vorticity [K], Q)`` of the rigid rotation: ``2 Omega`` and ``|Omega|^2``."""
    w = np.atleast_1d(np.asarray(omega, np.float64))
    return 2.0 * w, float((w * w).sum())


# per-env rotation rates and translations of the analytic cases: dyadic, so every field value is exact in fp32
RIGID_2D = [(0.75, (0.5, -0.25)), (-1.25, (0.125, 0.375))]
RIGID_3D = [((0.5, -0.75, 1.25), (0.25, -0.5, 0.125)), ((-1.0, 0.25, 0.5), (0.0, 0.375, -0.25))]


def rigid_single_case(dims: int) -> Case:
    """Uniform single-block grid, all faces FIXED, ``(9, 7)`` cells of 1/4 x 1/8 or ``(5, 4, 3)`` cells of 1/4 x 1/8 x 1/2; env b
    carries rotation b; prescribed faces carry the exact field at the face centres."""
    n = (9, 7) if dims == 2 else (5, 4, 3)
    h = (0.25, 0.125, 0.5)[:dims]
    widths = [np.full(n[a], h[a], np.float32) for a in range(dims)]
    edges = [np.concatenate([[0.0], np.cumsum(w.astype(np.float64))]) for w in widths]
    shape = tuple(reversed(n))
    centres = [0.5 * (e[1:] + e[:-1]) for e in edges]
    params = RIGID_2D if dims == 2 else RIGID_3D

    def points(axes_values):                                  # [d, *shape-like] from per-axis coordinate vectors (x, y(, z))
        mesh = np.meshgrid(*reversed(axes_values), indexing="ij")
        return np.stack([mesh[dims - 1 - a] for a in range(dims)])

    velocity = np.stack([rigid_rotation(points(centres), w, c) for w, c in params])
    bvel = {}
    for f in range(2 * dims):
        a = f >> 1
        vals = list(centres)
        vals[a] = np.array([edges[a][-1] if f & 1 else edges[a][0]])
        bvel[f] = np.stack([rigid_rotation(points(vals), w, c) for w, c in params])
    return Case(dims, shape, edges, widths, list(range(2 * dims)), len(params), 0.01, velocity, bvel)


def rigid_affine_spec():
    """Two blocks (4 x 5 and 3 x 5 cells) cut from one uniform lattice of spacing 1/4, mapped by the affine shear
    ``x = xi + eta / 2, y = xi / 4 + eta``; joined +x -> -x, every other face FIXED.  Returns ``(spec, fields)`` with ``fields[b] =
    (u [2, N], {(block, face): boundary values [2, face cells]})`` of env b: the exact rigid rotation at the cell / face centres."""
    nx1, nx2, ny, h = 4, 3, 5, 0.25
    xi, eta = np.meshgrid(h * np.arange(nx1 + nx2 + 1), h * np.arange(ny + 1))          # [ny + 1, nx + 1]
    coords = np.stack([xi + 0.5 * eta, 0.25 * xi + eta])
    spec = Spec(2, 0.01)
    spec.blocks = [coords[:, :, :nx1 + 1].copy(), coords[:, :, nx1:].copy()]
    spec.connections = [(0, 1, 1, 0, 2)]
    faces = [(0, 0), (0, 2), (0, 3), (1, 1), (1, 2), (1, 3)]
    spec.fixed = [(b, f, np.zeros((2, ny if f < 2 else spec.blocks[b].shape[2] - 1))) for b, f in faces]

    def cell_centres(c):
        return 0.25 * (c[:, 1:, 1:] + c[:, 1:, :-1] + c[:, :-1, 1:] + c[:, :-1, :-1])

    def face_centres(c, f):
        if f < 2:
            col = c[:, :, -1 if f else 0]
            return 0.5 * (col[:, 1:] + col[:, :-1])
        row = c[:, -1 if f == 3 else 0, :]
        return 0.5 * (row[:, 1:] + row[:, :-1])

    fields = []
    for w, c in RIGID_2D:
        u = np.concatenate([rigid_rotation(cell_centres(blk), w, c).reshape(2, -1) for blk in spec.blocks], axis=1)
        fields.append((u, {(b, f): rigid_rotation(face_centres(spec.blocks[b], f), w, c) for b, f in faces}))
    return spec, fields


def set_oracle_boundary(dom: mbo.Domain, values: dict) -> None:
    """Install ``{(block, face): [d, face cells]}`` as the prescribed velocities of an oracle domain."""
    for (b, f), v in values.items():
        assert dom.blocks[b].bounds[f].type == mbo.FIXED
        dom.blocks[b].bounds[f].velocity = np.asarray(v, np.float64).reshape(dom.d, -1).copy()


def rigid_bounds(A: np.ndarray, eps: float):
    """Bounds of the analytic case from the gradient bound ``|g - g_exact| <= 8 eps A`` (the stencil is exact for a linear field on an
    affine mesh, and the exact ``g`` is skew with ``|g| <= A``):
    vorticity ``g_ij - g_ji``: ``8 eps (A_ij + A_ji)`` of its terms + ``4 eps (|g_ij| + |g_ji|)`` of the subtraction  -> ``12 eps (A_ij + A_ji)``;
    Q, quadratic in g: ``sum |g| 8 eps A + 16 eps 0.5 sum g^2``                                               -> ``16 eps sum A^2``;
    strain norm (exactly 0): ``sqrt(2 sum S^2)`` with ``|S_ij| <= 4 eps (A_ij + A_ji)``, + ``8 eps sqrt(sum g^2)``   -> ``20 eps sqrt(sum A^2)``."""
    d = A.shape[0]
    pairs = [(1, 0)] if d == 2 else [(2, 1), (0, 2), (1, 0)]
    sum_A2 = (A * A).sum(axis=(0, 1))
    return (np.stack([12.0 * eps * (A[i, j] + A[j, i]) for i, j in pairs]), 16.0 * eps * sum_A2, 20.0 * eps * np.sqrt(sum_A2))
