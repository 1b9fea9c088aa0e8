"""NumPy fp64 restatement of the mesh probes and tracers of the multi-block domains (``fluidgym_amd/simulation/mb_tracers.py``,
``csrc/fg_mb_tracers.hip``), written from the definitions: the vertex tables, the locator, the sampler and
the advection step.  TEST INFRASTRUCTURE ONLY.

The tables are built another way than the library builds them: block vertices are merged by their coordinates (plus the two ends of
a periodic block axis, which are one vertex with two positions), and the stencils are gathered vertex by vertex in Python loops.  The
walk and the arithmetic follow the library's rule and order of operations, in fp64, on inputs rounded as the library sees them
(``dtype``)."""
import numpy as np

SLACK_FACTOR = 4.0            # four times the largest measured ratio (0.98)
NEWTON, ACCEPT = 8, 1e-9


def blend(a, b, w):
    w = np.asarray(w)
    while w.ndim < np.ndim(a):
        w = w[..., None]
    with np.errstate(invalid="ignore"):
        return np.where(w == 1.0, b, a + w * (b - a))


def map_jac(X, xi):
    """The cell map and its Jacobian ``J[:, a, b] = d x_a / d xi_b`` of cells with corners ``X [P, 2^d, d]`` at ``xi [P, d]``."""
    P, C, d = X.shape
    J = np.zeros((P, d, d))
    e0, e1 = blend(X[:, 0], X[:, 1], xi[:, 0]), blend(X[:, 2], X[:, 3], xi[:, 0])
    if d == 2:
        x = blend(e0, e1, xi[:, 1])
        J[:, :, 0] = blend(X[:, 1] - X[:, 0], X[:, 3] - X[:, 2], xi[:, 1])
        J[:, :, 1] = e1 - e0
        return x, J
    e2, e3 = blend(X[:, 4], X[:, 5], xi[:, 0]), blend(X[:, 6], X[:, 7], xi[:, 0])
    f0, f1 = blend(e0, e1, xi[:, 1]), blend(e2, e3, xi[:, 1])
    x = blend(f0, f1, xi[:, 2])
    J[:, :, 0] = blend(blend(X[:, 1] - X[:, 0], X[:, 3] - X[:, 2], xi[:, 1]), blend(X[:, 5] - X[:, 4], X[:, 7] - X[:, 6], xi[:, 1]), xi[:, 2])
    J[:, :, 1] = blend(e1 - e0, e3 - e2, xi[:, 2])
    J[:, :, 2] = f1 - f0
    return x, J


def solve(J, r):
    """``J^-1 r`` by cofactors, as the kernel writes it."""
    d = r.shape[1]
    with np.errstate(all="ignore"):
        if d == 2:
            det = J[:, 0, 0] * J[:, 1, 1] - J[:, 0, 1] * J[:, 1, 0]
            return np.stack([(r[:, 0] * J[:, 1, 1] - J[:, 0, 1] * r[:, 1]) / det, (J[:, 0, 0] * r[:, 1] - r[:, 0] * J[:, 1, 0]) / det], axis=1)
        j = lambda a, b: J[:, a, b]
        c00, c01, c02 = j(1, 1) * j(2, 2) - j(1, 2) * j(2, 1), j(1, 2) * j(2, 0) - j(1, 0) * j(2, 2), j(1, 0) * j(2, 1) - j(1, 1) * j(2, 0)
        det = j(0, 0) * c00 + j(0, 1) * c01 + j(0, 2) * c02
        c10, c11, c12 = j(0, 2) * j(2, 1) - j(0, 1) * j(2, 2), j(0, 0) * j(2, 2) - j(0, 2) * j(2, 0), j(0, 1) * j(2, 0) - j(0, 0) * j(2, 1)
        c20, c21, c22 = j(0, 1) * j(1, 2) - j(0, 2) * j(1, 1), j(0, 2) * j(1, 0) - j(0, 0) * j(1, 2), j(0, 0) * j(1, 1) - j(0, 1) * j(1, 0)
        return np.stack([(c00 * r[:, 0] + c10 * r[:, 1] + c20 * r[:, 2]) / det, (c01 * r[:, 0] + c11 * r[:, 1] + c21 * r[:, 2]) / det,
                         (c02 * r[:, 0] + c12 * r[:, 1] + c22 * r[:, 2]) / det], axis=1)


def newton(X, p, slack, iterations=NEWTON, stop=None):
    """Newton on the cell map from ``xi = 1/2``: at most 8 iterations, iterates clamped to ``[-1, 2]``, stopped per point once the step
    is below ``slack / 4``."""
    P, d = p.shape
    xi, live = np.full((P, d), 0.5), np.ones(P, bool)
    stop = slack / 4 if stop is None else stop
    for _ in range(iterations):
        i = np.nonzero(live)[0]
        if not len(i):
            break
        x, J = map_jac(X[i], xi[i])
        dx = solve(J, x - p[i])
        with np.errstate(invalid="ignore"):
            v = xi[i] - dx
            xi[i] = np.where(v < -1, -1.0, np.where(v > 2, 2.0, v))
            live[i[(np.abs(dx) < stop).all(axis=1)]] = False
    return xi


def clamp01(xi):
    with np.errstate(invalid="ignore"):
        return np.where(xi >= 0, np.where(xi <= 1, xi, 1.0), 0.0)


def weights(offsets):
    """``pinv([1 ... 1; d / R]) e_1`` where it solves ``sum w = 1, sum w d = 0`` to 1e-9, else inverse-distance weights."""
    d = np.asarray(offsets, np.float64)
    r = np.linalg.norm(d, axis=1)
    A = np.vstack([np.ones(len(d)), (d / r.max()).T])
    w = np.linalg.pinv(A)[:, 0]
    e1 = np.zeros(A.shape[0]); e1[0] = 1
    if np.abs(A @ w - e1).max() <= ACCEPT:
        return w, True
    return (1 / r) / (1 / r).sum(), False


class RefMesh:
    """The tables of a prepared multi-block domain (the host-only handle of ``tests/stub_mb.py`` will do), rounded to ``dtype``."""

    def __init__(self, dom, dtype=np.float64):
        d = self.dims = int(dom.dims)
        C = 1 << d
        self.N, self.NB = int(dom.n_cells), int(dom.n_boundary_faces)
        self.nbr = dom.neighbors().astype(np.int64)
        bcell, bface, _ = dom.boundary_tables()
        bits = [[(k >> a) & 1 for a in range(d)] for k in range(C)]
        # block vertices, their positions; the cells' corners
        pos, cell_bv, X = [], np.zeros((self.N, C), np.int64), np.zeros((self.N, C, d))
        same, voff = [], 0                                   # pairs of block vertices a periodic axis identifies
        self.fcode, shifts = np.zeros((2 * d, self.N), np.int64), []
        scale = max(float(np.abs(b.coords).max()) for b in dom.blocks)
        for blk in dom.blocks:
            co = np.asarray(blk.coords, np.float64)
            size = list(blk.size)
            vid = voff + np.arange(co[0].size).reshape(co.shape[1:])              # [(nz+1,) ny+1, nx+1]
            pos.append(co.reshape(d, -1).T)
            for c in range(blk.n_cells):
                ijk, rem = [], c
                for a in range(d):
                    ijk.append(rem % size[a]); rem //= size[a]
                for k in range(C):
                    at = tuple(ijk[a] + bits[k][a] for a in reversed(range(d)))
                    cell_bv[blk.cell_offset + c, k] = vid[at]
                    X[blk.cell_offset + c, k] = co[(slice(None),) + at]
                for a in blk.periodic_axes:
                    if ijk[a] == size[a] - 1:
                        self.fcode[2 * a + 1, blk.cell_offset + c] = -1 - a          # (the shift index is filled in below)
                    if ijk[a] == 0:
                        self.fcode[2 * a, blk.cell_offset + c] = -1 - a
            for a in blk.periodic_axes:
                ax = co.ndim - 1 - a
                first, last = np.take(co, 0, axis=ax), np.take(co, size[a], axis=ax)
                period = (last - first).reshape(d, -1)
                assert np.abs(period - period[:, :1]).max() <= 1e-6 * scale, "a periodic axis without one constant period"
                same.append((np.take(vid, 0, axis=ax - 1).reshape(-1), np.take(vid, size[a], axis=ax - 1).reshape(-1)))
                vec = period[:, 0]
                s = next((i for i, v in enumerate(shifts) if np.abs(v - vec).max() <= 1e-6 * scale), None)
                if s is None:
                    shifts.append(vec); s = len(shifts) - 1
                cells = slice(blk.cell_offset, blk.cell_offset + blk.n_cells)
                hi, lo = self.fcode[2 * a + 1, cells], self.fcode[2 * a, cells]
                hi[hi == -1 - a] = 1 + 2 * s            # through the high face: position -= period, crossing +1
                lo[lo == -1 - a] = 2 + 2 * s
            voff += co[0].size
        pos = np.concatenate(pos)
        # merge: equal coordinates, and the two ends of a periodic axis
        key = np.round(pos / (1e-6 * scale)).astype(np.int64)
        _, label = np.unique(key, axis=0, return_inverse=True)
        label = label.reshape(-1)
        for a_ids, b_ids in same:
            for i, j in zip(a_ids, b_ids):
                la, lb = label[i], label[j]
                if la != lb:
                    label[label == max(la, lb)] = min(la, lb)
        _, label = np.unique(label, return_inverse=True)
        self.cell_vert = label.reshape(-1)[cell_bv]
        self.V = int(self.cell_vert.max()) + 1
        self.X64 = X
        # stencils, vertex by vertex
        touching = [[] for _ in range(self.V)]            # (cell, offset centre - vertex)
        slots = [[] for _ in range(self.V)]               # (slot, offset face centre - vertex)
        centres = X.mean(axis=1)
        for c in range(self.N):
            for k in range(C):
                touching[self.cell_vert[c, k]].append((c, centres[c] - X[c, k]))
        for s, (c, f) in enumerate(zip(bcell, bface)):
            assert self.nbr[f, c] == -1 - s
            corners = [k for k in range(C) if bits[k][f >> 1] == (f & 1)]
            fc = X[c, corners].mean(axis=0)
            for k in corners:
                slots[self.cell_vert[c, k]].append((self.N + s, fc - X[c, k]))
        self.on_fixed = np.array([len(s) > 0 for s in slots])
        self.singular = np.array([not f and len(t) != C for t, f in zip(touching, self.on_fixed)])      # three or five cells meet (x span)
        Kv = max(len(s) if s else len(t) for s, t in zip(slots, touching))
        Kc = max(len(t) for t in touching)
        self.vel_idx, self.vel_w = np.zeros((self.V, Kv), np.int64), np.zeros((self.V, Kv))
        self.cell_idx, self.cell_w = np.zeros((self.V, Kc), np.int64), np.zeros((self.V, Kc))
        self.exact, self.cell_exact = np.zeros(self.V, bool), np.zeros(self.V, bool)
        self.n_touching = np.array([len(t) for t in touching])
        for v in range(self.V):
            w, ok = weights([o for _, o in touching[v]])
            self.cell_idx[v, :len(w)], self.cell_w[v, :len(w)], self.cell_exact[v] = [i for i, _ in touching[v]], w, ok
            if slots[v]:
                w, ok = weights([o for _, o in slots[v]])
                self.vel_idx[v, :len(w)], self.vel_w[v, :len(w)], self.exact[v] = [i for i, _ in slots[v]], w, ok
            else:
                self.vel_idx[v, :len(w)], self.vel_w[v, :len(w)], self.exact[v] = self.cell_idx[v, :len(w)], w, ok
        # slack
        shortest = np.full(self.N, np.inf)
        for k in range(C):
            for a in range(d):
                if not bits[k][a]:
                    shortest = np.minimum(shortest, np.linalg.norm(X[:, k | (1 << a)] - X[:, k], axis=1))
        self.mesh_ratio = float((np.abs(X).reshape(self.N, -1).max(axis=1) / shortest).max())
        self.shortest = shortest
        self.dtype = dtype
        self.slack = float(dtype(SLACK_FACTOR * np.finfo(dtype).eps * self.mesh_ratio))
        rnd = lambda a: np.asarray(a, np.float64).astype(dtype).astype(np.float64)
        self.X, self.vel_w, self.cell_w = rnd(X), rnd(self.vel_w), rnd(self.cell_w)
        self.shifts = rnd(np.array(shifts).reshape(-1, d))
        self.centres = centres
        self.extent = float((X.reshape(-1, d).max(0) - X.reshape(-1, d).min(0)).max())
        self.W = float(max(np.abs(self.vel_w).sum(axis=1).max(), np.abs(self.cell_w).sum(axis=1).max()))


def vertex_velocity(mesh, vel, bvel):
    """``[V, d]`` of a velocity ``[d, N]`` and boundary velocity ``[d, NB]``: the sum over the stencil in table order."""
    both = np.concatenate([vel, bvel[:, :mesh.NB]], axis=1)
    out = np.zeros((mesh.V, vel.shape[0]))
    for j in range(mesh.vel_w.shape[1]):
        use = mesh.vel_w[:, j] != 0
        out[use] += mesh.vel_w[use, j, None] * both[:, mesh.vel_idx[use, j]].T
    return out


def vertex_scalar(mesh, f):
    out = np.zeros(mesh.V)
    for j in range(mesh.cell_w.shape[1]):
        use = mesh.cell_w[:, j] != 0
        out[use] += mesh.cell_w[use, j] * f[mesh.cell_idx[use, j]]
    return out


def blend_corners(vals, xi):
    """Multilinear blend of corner values ``[P, 2^d(, k)]`` with ``xi [P, d]``: x first, then y, then z."""
    v = vals
    for a in range(xi.shape[1]):
        v = blend(v[:, 0::2], v[:, 1::2], xi[:, a])
    return v[:, 0]


def sample(mesh, vel, bvel, extras, cell, xi):
    """``[P, d + len(extras)]`` at the located points (cell clamped to the mesh, ``xi`` to the unit cube)."""
    cell = np.clip(np.asarray(cell, np.int64), 0, mesh.N - 1)
    xi = clamp01(np.asarray(xi, np.float64))
    cols = [blend_corners(vertex_velocity(mesh, vel, bvel)[mesh.cell_vert[cell]], xi)]
    for f in extras:
        cols.append(blend_corners(vertex_scalar(mesh, f)[mesh.cell_vert[cell]], xi)[:, None])
    return np.concatenate(cols, axis=1)


def locate(mesh, points, start, max_walk=256, q=None):
    """The walk.  Returns a dict: ``cell``, ``xi`` (clamped), ``status``, ``slot``, ``changes``, ``p`` (the points, shifted at periodic
    faces), ``q`` (a companion position shifted alike), ``wraps`` (signed crossings per shift vector)."""
    d, slack = mesh.dims, mesh.slack
    p = np.array(points, np.float64).reshape(-1, d)
    q = None if q is None else np.array(q, np.float64).reshape(-1, d)
    P = len(p)
    cell = np.clip(np.asarray(start, np.int64).reshape(-1), 0, mesh.N - 1).copy()
    prev, accept = np.full(P, -1, np.int64), np.zeros(P, bool)
    status, slot, changes = np.full(P, 2, np.int64), np.zeros(P, np.int64), np.zeros(P, np.int64)
    xi, wr, active = np.zeros((P, d)), np.zeros((P, len(mesh.shifts)), np.int64), np.ones(P, bool)
    while active.any():
        idx = np.nonzero(active)[0]
        x_i = newton(mesh.X[cell[idx]], p[idx], slack)
        xi[idx] = x_i
        with np.errstate(invalid="ignore"):
            nan = np.isnan(x_i).any(axis=1)
            inside = ((x_i >= -slack) & (x_i <= 1 + slack)).all(axis=1)
        ok = ~nan & (inside | accept[idx])
        status[idx[ok]] = 0
        active[idx[nan | ok]] = False
        idx, x_i = idx[~(nan | ok)], x_i[~(nan | ok)]
        if not len(idx):
            continue
        n = len(idx)
        viol = np.empty((n, 2 * d))
        viol[:, 0::2], viol[:, 1::2] = -x_i, x_i - 1
        tried, searching = np.zeros((n, 2 * d), bool), np.ones(n, bool)
        nxt, code, first_slot = np.full(n, -1, np.int64), np.zeros(n, np.int64), np.full(n, -1, np.int64)
        for _ in range(2 * d):
            v = np.where(tried, -np.inf, viol)
            best = v.argmax(axis=1)                      # the first of equals: the lower face index
            searching &= v[np.arange(n), best] > slack
            rows = np.nonzero(searching)[0]
            if not len(rows):
                break
            tried[rows, best[rows]] = True
            nb = mesh.nbr[best[rows], cell[idx[rows]]]
            go = nb >= 0
            nxt[rows[go]] = nb[go]
            code[rows[go]] = mesh.fcode[best[rows[go]], cell[idx[rows[go]]]]
            searching[rows[go]] = False
            fx, fnb = rows[~go], nb[~go]
            new = first_slot[fx] < 0
            first_slot[fx[new]] = -1 - fnb[new]
        out = nxt < 0
        status[idx[out]] = 1
        slot[idx[out]] = np.clip(first_slot[out], 0, max(mesh.NB - 1, 0))
        active[idx[out]] = False
        spent = ~out & (changes[idx] >= max_walk)
        active[idx[spent]] = False
        mv = ~out & ~spent
        j, c = idx[mv], code[mv]
        changes[j] += 1
        has = c > 0
        s, back = (c[has] - 1) >> 1, ((c[has] - 1) & 1) == 1
        move = np.where(back, 1.0, -1.0)[:, None] * mesh.shifts[s]
        p[j[has]] += move
        if q is not None:
            q[j[has]] += move
        wr[j[has], s] += np.where(back, -1, 1)
        accept[j] = nxt[mv] == prev[j]
        prev[j] = cell[j]
        cell[j] = nxt[mv]
    return dict(cell=cell, xi=clamp01(xi), raw_xi=xi, status=status, slot=slot, changes=changes, p=p, q=q, wraps=wr)


def advect(mesh, vel, bvel, respawn_slots, seed_pos, seed_cell, pos, cell, age, wraps, dt, substeps, walk=64):
    """``substeps`` midpoint steps.  Returns ``(pos, cell, age, wraps, lost, margin)``; ``margin [n]`` is the smallest distance in ``xi`` from a
    cell face over all positions the call located for the tracer (for the tests that compare two precisions)."""
    dtype, d = mesh.dtype, mesh.dims
    x, c = np.array(pos, np.float64), np.clip(np.asarray(cell, np.int64), 0, mesh.N - 1).copy()
    seed_pos, seed_cell = np.asarray(seed_pos, np.float64), np.clip(np.asarray(seed_cell, np.int64), 0, mesh.N - 1)
    n = len(x)
    wr = np.array(wraps, np.int64).reshape(n, -1).copy()
    h = float(dtype(dt) / dtype(substeps))
    half = float(dtype(0.5) * dtype(h))
    xi, have, reborn = np.zeros((n, d)), np.zeros(n, bool), np.zeros(n, bool)
    margin, lost = np.full(n, np.inf), 0
    respawn_slots = np.asarray(respawn_slots)
    vv = vertex_velocity(mesh, vel, bvel)
    velocity = lambda cc, xx: blend_corners(vv[mesh.cell_vert[cc]], xx)

    def note(i, r):
        m = np.minimum(r["raw_xi"], 1 - r["raw_xi"]).min(axis=1)
        margin[i] = np.minimum(margin[i], np.where(r["status"] == 0, m, 0.0))

    def settle(i, status, slot):
        nonlocal lost
        lost += int((status == 2).sum())
        resp = (status == 2) | ((status == 1) & (respawn_slots[slot] != 0))
        on = (status == 1) & ~resp
        if on.any():
            x[i[on]] = map_jac(mesh.X[c[i[on]]], xi[i[on]])[0]
        r = i[resp]
        reborn[r] = True
        c[r], x[r], wr[r] = seed_cell[r], seed_pos[r], 0
        return ~resp

    for _ in range(substeps):
        i = np.nonzero(~have & ~reborn)[0]           # (a respawn ends the call for the tracer: it rests at its seed)
        if len(i):
            r = locate(mesh, x[i], c[i], walk)
            x[i], c[i], xi[i] = r["p"], r["cell"], r["xi"]
            wr[i] += r["wraps"]
            note(i, r)
            have[i] = settle(i, r["status"], r["slot"])
            moved = i[~have[i]]
        else:
            moved = i
        i = np.setdiff1d(np.nonzero(have)[0], moved)
        if not len(i):
            continue
        with np.errstate(all="ignore"):
            xs = x[i] + half * velocity(c[i], xi[i])
        fin = np.isfinite(xs).all(axis=1)
        status, slot = np.full(len(i), 2, np.int64), np.zeros(len(i), np.int64)
        k = i[fin]
        r = locate(mesh, xs[fin], c[k], walk, q=x[k])
        x[k] = r["q"]
        wr[k] += r["wraps"]
        note(k, r)
        status[fin] = r["status"]
        g = r["status"] != 2
        kg = k[g]
        with np.errstate(all="ignore"):
            x[kg] += h * velocity(r["cell"][g], r["xi"][g])
        c[kg] = r["cell"][g]
        fin2 = np.isfinite(x[kg]).all(axis=1)
        st2, sl2 = np.full(len(kg), 2, np.int64), np.zeros(len(kg), np.int64)
        kf = kg[fin2]
        r2 = locate(mesh, x[kf], c[kf], walk)
        x[kf], c[kf], xi[kf] = r2["p"], r2["cell"], r2["xi"]
        wr[kf] += r2["wraps"]
        note(kf, r2)
        st2[fin2], sl2[fin2] = r2["status"], r2["slot"]
        pos_in_i = np.nonzero(fin)[0][g]
        status[pos_in_i], slot[pos_in_i] = st2, sl2
        slot[np.nonzero(fin)[0][~g]] = 0
        have[i] = settle(i, status, slot)
    age = np.where(reborn, 0.0, (np.asarray(age).astype(dtype) + dtype(dt)).astype(np.float64))
    return x, c, age, wr, lost, margin
