"""NumPy fp64 restatement of the interpolant and the tracer advection of ``fg_point_sample`` / ``fg_tracer_advect`` -- TEST
INFRASTRUCTURE ONLY, written from the specification (include/fluidgym_hip.h), not from the kernels.

One env at a time.  Fields are ``[d, (Z,) Y, X]`` / ``[(Z,) Y, X]`` arrays, boundary velocities ``{face: [d, (Z,) Y, X]}`` with extent 1
along the normal axis (face = 2 * axis + side, axes x, y, z).  Everything is computed in fp64 whatever dtype the inputs have, so a
comparison with the fp32 library runs this on the same fp32 inputs."""
import numpy as np


def node_arrays(edges, periodic):
    """Per axis the fp64 nodes: the centres (periodic) or low face, centres, high face (FIXED)."""
    out = []
    for e, per in zip(edges, periodic):
        e = np.asarray(e, np.float64)
        c = 0.5 * (e[:-1] + e[1:])
        out.append(c if per else np.concatenate([[e[0]], c, [e[-1]]]))
    return out


class RefGrid:
    def __init__(self, nodes, periodic, lo, length):
        self.periodic = [bool(p) for p in periodic]
        self.nodes = [np.asarray(n, np.float64) for n in nodes]
        self.lo = np.asarray(lo, np.float64)
        self.len = np.asarray(length, np.float64)
        self.dims = len(self.nodes)
        self.n = [len(n) - (0 if p else 2) for n, p in zip(self.nodes, self.periodic)]

    @classmethod
    def from_edges(cls, edges, periodic, dtype=np.float64):
        """The grid the library sees: nodes, lo and length computed in fp64 and rounded to ``dtype``."""
        nodes = [n.astype(dtype) for n in node_arrays(edges, periodic)]
        lo = np.array([np.asarray(e, np.float64)[0] for e in edges]).astype(dtype)
        length = np.array([np.asarray(e, np.float64)[-1] - np.asarray(e, np.float64)[0] for e in edges]).astype(dtype)
        return cls(nodes, periodic, lo, length)


def blend(a, b, w):
    with np.errstate(invalid="ignore"):
        return np.where(w == 1.0, b, a + w * (b - a))


def wrap(x, lo, length):
    """``x`` in ``[lo, lo + length)`` and the signed number of periods taken off."""
    with np.errstate(invalid="ignore"):
        q = np.floor((x - lo) / length)
        x = x - q * length
        k = np.where(np.isnan(q), 0, q).astype(np.int64)
        low = x < lo
        x = np.where(low, x + length, x)
        k = k - low
        high = x >= lo + length
        x = np.where(high, x - length, x)
        k = k + high
    return x, k


def locate(grid, a, x):
    """Corners of axis ``a`` at the positions ``x``: cell indices ``c0, c1``, faces ``f0, f1`` (-1 a centre, 0 / 1 the low / high face), ``w``."""
    nodes, n, lo, length = grid.nodes[a], grid.n[a], grid.lo[a], grid.len[a]
    m = len(nodes)
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore"):
        if grid.periodic[a]:
            x, _ = wrap(x, lo, length)
        else:
            x = np.where(x < nodes[0], nodes[0], np.where(x > nodes[-1], nodes[-1], x))        # the face nodes
        k = np.where(np.isnan(x), 0, np.searchsorted(nodes, x, side="right"))      # how many nodes are <= x (none for a NaN)
        if grid.periodic[a]:
            c0, c1 = np.where(k == 0, m - 1, k - 1), np.where(k >= m, 0, k)
            x0 = np.where(k == 0, nodes[m - 1] - length, nodes[np.maximum(k - 1, 0)])
            x1 = np.where(k >= m, nodes[0] + length, nodes[np.minimum(k, m - 1)])
            f0 = f1 = np.full(x.shape, -1)
        else:
            j = np.clip(k - 1, 0, m - 2)
            f0, f1 = np.where(j == 0, 0, -1), np.where(j + 1 == m - 1, 1, -1)
            c0, c1 = np.maximum(j - 1, 0), np.minimum(j, n - 1)
            x0, x1 = nodes[j], nodes[j + 1]
        w = (x - x0) / (x1 - x0)
    return c0, c1, f0, f1, w


def _as3d(grid, field):
    """``[C, Z, Y, X]`` view of a ``[C, (Z,) Y, X]`` array."""
    f = np.asarray(field, np.float64)
    return f[:, None] if grid.dims == 2 else f


def _corners(grid, points):
    pts = np.asarray(points, np.float64)
    loc = [locate(grid, a, pts[:, a]) for a in range(grid.dims)]
    if grid.dims == 2:
        zero = np.zeros(len(pts), np.int64)
        loc.append((zero, zero, zero - 1, zero - 1, np.zeros(len(pts))))
    return loc


def sample_velocity(grid, velocity, bvel, points):
    """The velocity ``[P, d]`` at ``points`` ``[P, d]``."""
    d = grid.dims
    vel = _as3d(grid, velocity)
    bv = {f: _as3d(grid, t) for f, t in bvel.items()}
    (x0, x1, fx0, fx1, wx), (y0, y1, fy0, fy1, wy), (z0, z1, fz0, fz1, wz) = _corners(grid, points)

    def corner(cx, fx, cy, fy, cz, fz):
        out = vel[:, cz, cy, cx]                                       # [d, P]
        for axis, f, index in ((2, fz, lambda t: t[:, 0, cy, cx]), (0, fx, lambda t: t[:, cz, cy, 0]), (1, fy, lambda t: t[:, cz, 0, cx])):
            # applied z, x, y: the last one applied wins, so the priority is y, then x, then z
            for side in (0, 1):
                face = 2 * axis + side
                if face in bv:
                    out = np.where(f == side, index(bv[face]), out)
        return out

    def along_x(cy, fy, cz, fz):
        return blend(corner(x0, fx0, cy, fy, cz, fz), corner(x1, fx1, cy, fy, cz, fz), wx)

    def along_y(cz, fz):
        return blend(along_x(y0, fy0, cz, fz), along_x(y1, fy1, cz, fz), wy)

    out = along_y(z0, fz0) if d == 2 else blend(along_y(z0, fz0), along_y(z1, fz1), wz)
    return out.T


def sample_scalar(grid, field, points):
    """A cell-centred field without face values ``[P]``: a face node reads the adjacent cell."""
    f = _as3d(grid, np.asarray(field, np.float64)[None])[0]
    (x0, x1, _, _, wx), (y0, y1, _, _, wy), (z0, z1, _, _, wz) = _corners(grid, points)
    along_y = lambda cz: blend(blend(f[cz, y0, x0], f[cz, y0, x1], wx), blend(f[cz, y1, x0], f[cz, y1, x1], wx), wy)
    return along_y(z0) if grid.dims == 2 else blend(along_y(z0), along_y(z1), wz)


def advect(grid, velocity, bvel, seed, pos, age, wraps, dt, substeps, respawn_faces=0):
    """One ``fg_tracer_advect`` call for one env: ``(pos, age, wraps, lost)`` after ``substeps`` midpoint steps of ``dt / substeps``."""
    d = grid.dims
    x = np.array(pos, np.float64)
    seed = np.asarray(seed, np.float64)
    wr = np.array(wraps, np.int64)
    h = float(dt) / substeps
    reborn = np.zeros(len(x), bool)
    lost = 0
    for _ in range(substeps):
        u = sample_velocity(grid, velocity, bvel, x)
        xs = x + 0.5 * h * u
        with np.errstate(invalid="ignore", over="ignore"):
            x = x + h * sample_velocity(grid, velocity, bvel, xs)
        finite = np.isfinite(x).all(axis=1)
        lost += int((~finite).sum())
        respawn = ~finite
        for a in range(d):
            lo, hi = (grid.lo[a], grid.lo[a] + grid.len[a]) if grid.periodic[a] else (grid.nodes[a][0], grid.nodes[a][-1])
            if grid.periodic[a]:
                xa, k = wrap(np.where(finite, x[:, a], lo), lo, grid.len[a])
                x[:, a] = np.where(finite, xa, x[:, a])
                wr[:, a] += np.where(finite, k, 0)
            else:
                below, above = finite & (x[:, a] < lo), finite & (x[:, a] > hi)
                if (respawn_faces >> (2 * a)) & 1:
                    respawn |= below
                else:
                    x[:, a] = np.where(below, lo, x[:, a])
                if (respawn_faces >> (2 * a + 1)) & 1:
                    respawn |= above
                else:
                    x[:, a] = np.where(above, hi, x[:, a])
        x[respawn] = seed[respawn]
        wr[respawn] = 0
        reborn |= respawn
    return x, np.where(reborn, 0.0, np.asarray(age, np.float64) + dt), wr, lost
