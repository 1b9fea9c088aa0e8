"""CPU-side checks of the mesh probes and tracers of the multi-block domains (``fluidgym_amd/simulation/mb_tracers.py``,
``csrc/fg_mb_tracers.hip``).  Part 1 holds the host tables and the NumPy restatement the GPU tests compare
against (``tests/mb_tracers_ref.py``) to facts of the meshes; part 2 holds the three entry points to their argument checks, which
answer before any launch, and the env interface to its refusals.  The meshes come from the host-only handle of ``tests/stub_mb.py``."""
import ctypes
import os
import re

import numpy as np
import pytest

from fluidgym_amd import _lib as L
from fluidgym_amd.simulation import mb_tracers as M
from tests import helpers_mb as H
from tests import mb_tracers_ref as R
from tests import stub_mb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fg_mb_point_locate", "fg_mb_point_sample", "fg_mb_tracer_advect")
MESHES = {"cylinder_2d": lambda: H.cylinder_2d(8), "airfoil": lambda: H.airfoil_spec(4), "twisted_ring": H.twisted_ring,
          "skewed_pair": H.skewed_pair, "split_rotated_channel": H.split_rotated_channel, "skewed_pair_3d": H.skewed_pair_3d,
          "cylinder_3d_small": H.cylinder_3d_small}
EULER = {"cylinder_2d": 0, "airfoil": 0, "twisted_ring": 0, "skewed_pair": 1, "split_rotated_channel": 1}
EXTRUDED = {"skewed_pair_3d": ("skewed_pair", 3), "cylinder_3d_small": (lambda: H.cylinder_2d(4), 3)}
_CACHE = {}


def case(name):
    """(domain, library tables, restatement) of a mesh, built once."""
    if name not in _CACHE:
        restore = stub_mb.install()
        try:
            dom = MESHES[name]().native()
            _CACHE[name] = (dom, M.domain_point_tables(dom), R.RefMesh(dom))
        finally:
            restore()
    return _CACHE[name]


def random_points(T, n, rng, cells=None):
    cells = rng.integers(0, T.n_cells, n) if cells is None else cells[rng.integers(0, len(cells), n)]
    xi = rng.random((n, T.dims))
    return cells, xi, M.cell_map(T.cell_xyz[cells], xi)


# ------------------------------------------------------------------------------------------------ part 1: tables and restatement
@pytest.mark.parametrize("name", list(MESHES))
def test_topology(name):
    dom, T, ref = case(name)
    d = T.dims
    assert T.n_vertices == ref.V                          # union-find over shared faces == merging by coordinates (+ periodic ends)
    if d == 2:
        E = (2 * d * T.n_cells + T.n_slots) // 2
        assert T.n_vertices - E + T.n_cells == EULER[name]
        if name == "cylinder_2d":
            assert (T.n_vertices, E, T.n_cells) == (2204, 4188, 1984)
    else:
        base, nz = EXTRUDED[name]
        restore = stub_mb.install()
        try:
            flat = M.domain_point_tables((MESHES[base] if isinstance(base, str) else base)().native())
        finally:
            restore()
        assert T.n_vertices == nz * flat.n_vertices       # the two z ends are one vertex with two positions
        assert len(T.shifts) == 1 and T.shifts[0, 2] != 0 and not T.shifts[0, :2].any()
    # the same vertices, whatever they are called: cells share a library vertex exactly where they share a restated one
    a, b = T.cell_vert.reshape(-1), ref.cell_vert.reshape(-1)
    pairs = np.unique(np.stack([a, b]), axis=1)
    assert pairs.shape[1] == T.n_vertices
    assert np.array_equal(T.face_code, ref.fcode) and np.allclose(np.abs(T.shifts), np.abs(ref.shifts), atol=0, rtol=1e-15)
    assert T.mesh_ratio == pytest.approx(ref.mesh_ratio, rel=1e-14) and M.SLACK_FACTOR == R.SLACK_FACTOR
    assert T.slack(np.float32) == pytest.approx(np.float32(ref.mesh_ratio * 4 * np.finfo(np.float32).eps), rel=1e-6)


@pytest.mark.parametrize("name", list(MESHES))
def test_weights(name):
    dom, T, ref = case(name)
    assert np.abs(T.vel_w.sum(axis=1) - 1).max() < 1e-12 and np.abs(T.cell_w.sum(axis=1) - 1).max() < 1e-12
    assert T.exact[~T.on_fixed].all() and T.cell_exact[~T.on_fixed].all()
    assert np.array_equal(T.on_fixed, ref.on_fixed[_vertex_map(T, ref)]) and np.array_equal(T.exact, ref.exact[_vertex_map(T, ref)])
    # zero first moment: offsets centre - vertex as the touching cell stores the vertex
    centres = T.cell_xyz.mean(axis=1)
    moment, radius = np.zeros((T.n_vertices, T.dims)), np.zeros(T.n_vertices)
    weight_of = {}
    for v in range(T.n_vertices):
        for j in range(T.cell_idx.shape[1]):
            if T.cell_w[v, j] != 0:
                weight_of[(v, int(T.cell_idx[v, j]))] = T.cell_w[v, j]
    for c in range(T.n_cells):
        for k in range(1 << T.dims):
            v = int(T.cell_vert[c, k])
            off = centres[c] - T.cell_xyz[c, k]
            moment[v] += weight_of[(v, c)] * off
            radius[v] = max(radius[v], np.linalg.norm(off))
    free = ~T.on_fixed
    assert (np.abs(moment[free]).max(axis=1) <= 1e-9 * radius[free]).all()
    assert T.vel_w.min() < 0 or name not in ("cylinder_2d", "airfoil")               # nothing promises monotonicity
    # the vertex values of the two table sets agree for random fields
    rng = np.random.default_rng(3)
    vel, bvel = rng.standard_normal((T.dims, T.n_cells)), rng.standard_normal((T.dims, max(T.n_slots, 1)))
    mine = _as_ref(T)
    assert np.abs(R.vertex_velocity(mine, vel, bvel)[T.cell_vert] - R.vertex_velocity(ref, vel, bvel)[ref.cell_vert]).max() < 1e-12
    assert np.abs(R.vertex_scalar(mine, vel[0])[T.cell_vert] - R.vertex_scalar(ref, vel[0])[ref.cell_vert]).max() < 1e-12


def _vertex_map(T, ref):
    m = np.zeros(T.n_vertices, np.int64)
    m[T.cell_vert.reshape(-1)] = ref.cell_vert.reshape(-1)
    return m


def _as_ref(T):
    class Tables:
        pass

    t = Tables()
    t.V, t.N, t.NB, t.vel_idx, t.vel_w, t.cell_idx, t.cell_w = T.n_vertices, T.n_cells, T.n_slots, T.vel_idx, T.vel_w, T.cell_idx, T.cell_w
    return t


@pytest.mark.parametrize("name", list(MESHES))
def test_affine_fields_are_reproduced(name):
    dom, T, ref = case(name)
    d = T.dims
    rng = np.random.default_rng(11)
    A, b = rng.standard_normal((d + 1, d)), rng.standard_normal(d + 1)
    centres = ref.X64.mean(axis=1)
    bcell, bface, _ = dom.boundary_tables()
    fc = np.array([ref.X64[c, [k for k in range(1 << d) if ((k >> (f >> 1)) & 1) == (f & 1)]].mean(axis=0) for c, f in zip(bcell, bface)])
    field = lambda x: x @ A.T + b
    vel, bvel, p = field(centres)[:, :d].T, field(fc)[:, :d].T, field(centres)[:, d]
    # every cell without a vertex on a FIXED face, none left out -- except, on a periodic mesh, the cells with a vertex on the periodic
    # seam: an affine field is not periodic, the stencil of such a vertex reads centres one period apart (as on the single-block grids)
    seam = np.zeros(ref.V, bool)
    for f in range(2 * d):
        corners = [k for k in range(1 << d) if ((k >> (f >> 1)) & 1) == (f & 1)]
        seam[ref.cell_vert[ref.fcode[f] > 0][:, corners].reshape(-1)] = True
    assert seam.any() == (len(ref.shifts) > 0)
    inner = np.nonzero(~(ref.on_fixed | seam)[ref.cell_vert].any(axis=1))[0]
    assert len(inner) > 0
    # the cells at vertices where another number of cells meet than 2^d are part of the set wherever the mesh has such a vertex off
    # the FIXED faces; on the cylinder and airfoil meshes the three-cell vertices exist (asserted) and lie on the boundary
    if name in ("cylinder_2d", "airfoil"):
        assert (ref.n_touching == 3).any() or (ref.n_touching == 5).any()
    cells, xi, pts = random_points(T, 2000, rng, inner)
    got = R.sample(ref, vel, bvel, [p], cells, xi)
    scale = np.abs(field(pts)).max()
    # 1e-12 F where the blocks store one position per shared vertex (every mesh here but cylinder_3d_small, whose generator rounds the
    # two copies of a seam vertex to fp32 separately: they differ by delta = one fp32 ulp).  The offsets are taken from the vertex as
    # the touching cell's block stores it, so with sum w d = 0 a vertex value is the field at sum_k w_k x_v^(k), a point within
    # sum |w| delta of every copy: the interpolant then reproduces the field to |grad| W delta per coordinate and no better.
    lo, hi = np.full((ref.V, d), np.inf), np.full((ref.V, d), -np.inf)
    np.minimum.at(lo, ref.cell_vert.reshape(-1), ref.X64.reshape(-1, d)); np.maximum.at(hi, ref.cell_vert.reshape(-1), ref.X64.reshape(-1, d))
    delta = float((hi - lo)[~seam].max())
    assert delta < 1e-15 or name == "cylinder_3d_small"        # (the ring closes on itself at cos / sin of 2 pi: 1e-16)
    tol = 1e-12 * scale + np.abs(A).sum(axis=1).max() * ref.W * delta
    assert np.abs(got - field(pts)).max() <= tol
    got = R.sample(_with_tables(ref, T), vel, bvel, [p], cells, xi)                  # and with the library's tables
    assert np.abs(got - field(pts)).max() <= tol


def _with_tables(ref, T):
    import copy

    m = copy.copy(ref)
    m.V, m.cell_vert, m.vel_idx, m.vel_w, m.cell_idx, m.cell_w = T.n_vertices, T.cell_vert, T.vel_idx, T.vel_w, T.cell_idx, T.cell_w
    return m


@pytest.mark.parametrize("name", list(MESHES))
def test_location(name):
    dom, T, ref = case(name)
    rng = np.random.default_rng(21)
    cells, xi, pts = random_points(T, 4000, rng)
    r = R.locate(ref, pts, M.nearest_cells(T.centres, pts))
    assert (r["status"] == 0).all() and r["changes"].max() <= 8
    back = R.map_jac(ref.X[r["cell"]], r["xi"])[0]
    assert np.abs(back - r["p"]).max() <= 1e-12 * ref.extent
    # outside, beyond a wall, and a NaN
    far = T.bounds[1] + 0.3 * (T.bounds[1] - T.bounds[0])
    r = R.locate(ref, np.stack([far, np.full(T.dims, np.nan)]), np.zeros(2, np.int64))
    assert r["status"].tolist()[1] == 2 and r["status"][0] in (1, 2) and np.isfinite(r["xi"]).all()
    assert (M.nearest_cells(T.centres, np.full((1, T.dims), np.nan)) == 0).all()


@pytest.mark.parametrize("name", list(MESHES))
def test_continuity_across_every_shared_face(name):
    dom, T, ref = case(name)
    d = T.dims
    rng = np.random.default_rng(31)
    vel, bvel, p = rng.standard_normal((d, T.n_cells)), rng.standard_normal((d, max(T.n_slots, 1))), rng.standard_normal(T.n_cells)
    F = max(np.abs(vel).max(), np.abs(p).max())
    worst, crossed = 0.0, 0
    C = 1 << d
    bits = np.array([[(k >> a) & 1 for a in range(d)] for k in range(C)], np.float64)
    for f in range(2 * d):
        a, side = f >> 1, f & 1
        cells = np.nonzero(ref.nbr[f] >= 0)[0]
        nb = ref.nbr[f, cells]
        xi = rng.random((len(cells), d))
        xi[:, a] = side
        here = R.sample(ref, vel, bvel, [p], cells, xi)
        # the same point in the neighbour's coordinates: the corners of the shared face carry the same vertices in both cells, so
        # xi' = sum_k N_k(xi) bits(corner of the neighbour with the vertex of corner k) -- whatever way the neighbour is turned
        xin = np.zeros_like(xi)
        for k in [k for k in range(C) if ((k >> a) & 1) == side]:
            shape = np.prod(np.where(bits[k] == 1, xi, 1 - xi)[:, [b for b in range(d) if b != a]], axis=1)
            same = ref.cell_vert[nb] == ref.cell_vert[cells, k][:, None]
            assert (same.sum(axis=1) == 1).all()
            xin += shape[:, None] * bits[same.argmax(axis=1)]
        there = R.sample(ref, vel, bvel, [p], nb, xin)
        worst = max(worst, np.abs(here - there).max())
        crossed += int((ref.fcode[f, cells] > 0).sum())
        # and in physical space the two cells put that point in the same place, up to the periodic shift and the stored copies
        code = ref.fcode[f, cells]
        s, back = np.maximum((code - 1) >> 1, 0), ((code - 1) & 1) == 1
        shift = (np.where(back, 1.0, -1.0)[:, None] * ref.shifts[s] if len(ref.shifts) else np.zeros((len(cells), d))) * (code > 0)[:, None]
        gap = R.map_jac(ref.X[nb], xin)[0] - (R.map_jac(ref.X[cells], xi)[0] + shift)
        assert np.abs(gap).max() <= 2e-7 * ref.extent
    assert worst <= 1e-12 * F
    assert (crossed > 0) == (len(ref.shifts) > 0)


def test_seeds_lie_in_cells_and_do_not_depend_on_the_batch():
    dom, T, ref = case("cylinder_2d")
    c2, x2 = M.seed_cells_and_xi(5, 2, 64, T.volumes, 2)
    c5, x5 = M.seed_cells_and_xi(5, 5, 64, T.volumes, 2)
    assert np.array_equal(c2, c5[:2]) and np.array_equal(x2, x5[:2]) and not np.array_equal(c5[0], c5[1])
    r = np.random.default_rng([5, 1]).random((64, 3))
    assert np.array_equal(x2[1], r[:, 1:]) and (x2 >= 0).all() and (x2 < 1).all()
    cum = np.cumsum(T.volumes) / T.volumes.sum()
    assert np.array_equal(c2[1], np.minimum(np.searchsorted(cum, r[:, 0], side="right"), T.n_cells - 1))
    # the volume of a bilinear cell is |det J| at its centre: the shoelace area
    X = T.cell_xyz
    quad = X[:, [0, 1, 3, 2]]
    area = 0.5 * np.abs((quad[:, :, 0] * np.roll(quad[:, :, 1], -1, axis=1) - np.roll(quad[:, :, 0], -1, axis=1) * quad[:, :, 1]).sum(axis=1))
    assert np.allclose(T.volumes, area, rtol=1e-12)
    w, ok = M.vertex_weights(np.array([[1.0, 0.0], [-2.0, 0.0]]))                    # two points: linear interpolation along the chord
    assert ok and np.allclose(w, [2 / 3, 1 / 3])
    w, ok = M.vertex_weights(np.array([[1.0, 0.0], [0.0, 2.0]]))                     # no solution: inverse-distance weights
    assert not ok and np.allclose(w, [2 / 3, 1 / 3])


# ------------------------------------------------------------------------------------------------ part 2: the library, the envs
def test_both_libraries_export_the_entry_points():
    header = open(os.path.join(ROOT, "include", "fluidgym_hip.h")).read()
    mk = open(os.path.join(ROOT, "fluidgym_amd", "csrc", "Makefile")).read()
    assert all("fg_mb_tracers.hip" in line for line in mk.splitlines() if line.startswith(("SRCS =", "F64_SRCS =")))
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header)
        assert name in L.SIGNATURES and name in L.SIGNATURES_F64
        assert hasattr(L.load(), name) and hasattr(L.load_f64(), name)
    body = re.search(r"typedef struct fg_mb_point_mesh \{(.*?)\} fg_mb_point_mesh;", header, re.S).group(1)
    names = []
    for decl in body.split(";"):
        if decl.strip():
            names += [re.match(r"\W*(\w+)", x).group(1) for x in decl.strip().rsplit("*", 1)[-1].split(None, 1)[-1].split(",")]
    assert names == [f[0] for f in L.FgMbPointMesh._fields_] == [f[0] for f in L.FgMbPointMeshF64._fields_]
    assert dict(L.FgMbPointMeshF64._fields_)["slack"] is ctypes.c_double and dict(L.FgMbPointMesh._fields_)["slack"] is ctypes.c_float
    assert L.SIGNATURES_F64["fg_mb_tracer_advect"][1][1] is ctypes.c_double
    import fluidgym_amd

    assert fluidgym_amd.MeshProbes is M.MeshProbes and fluidgym_amd.MeshTracerCloud is M.MeshTracerCloud


ONE = 4096                  # a "device pointer" that is never dereferenced: every call below fails its argument checks first


def _mesh(lib_name, d=2, **change):
    m = (L.FgMbPointMesh if lib_name == "fp32" else L.FgMbPointMeshF64)()
    m.dims, m.batch, m.n_cells, m.n_slots, m.n_vertices, m.kv, m.kc, m.n_shifts = d, 2, 96, 40, 117, 4, 4, 1
    for name in ("cell_vert", "cell_xyz", "neighbors", "face_code", "vel_idx", "vel_w", "cell_idx", "cell_w", "velocity", "bvel"):
        setattr(m, name, ONE)
    m.slack = 1e-4
    m.velocity_stride, m.bvel_stride, m.bvel_comp_stride = d * 96, d * 40, 40
    for k, v in change.items():
        if isinstance(v, tuple):
            getattr(m, k)[v[0]] = v[1]
        else:
            setattr(m, k, v)
    return m


MESH_FAULTS = {
    "dims 1": dict(dims=1), "dims 4": dict(dims=4), "batch 0": dict(batch=0), "batch above 65535": dict(batch=65536), "n_cells 0": dict(n_cells=0),
    "n_slots negative": dict(n_slots=-1), "n_vertices 0": dict(n_vertices=0), "kv 0": dict(kv=0), "kc negative": dict(kc=-2),
    "n_shifts negative": dict(n_shifts=-1), "null cell_vert": dict(cell_vert=None), "null cell_xyz": dict(cell_xyz=None),
    "null neighbors": dict(neighbors=None), "null face_code": dict(face_code=None), "null vel_idx": dict(vel_idx=None), "null vel_w": dict(vel_w=None),
    "null cell_idx": dict(cell_idx=None), "null cell_w": dict(cell_w=None), "slack 0": dict(slack=0.0), "slack NaN": dict(slack=float("nan")),
    "slack 0.3": dict(slack=0.3), "shift infinite": dict(shifts=(1, float("inf"))), "null velocity": dict(velocity=None), "null bvel": dict(bvel=None),
    "short velocity stride": dict(velocity_stride=191), "short boundary stride": dict(bvel_stride=79), "short component stride": dict(bvel_comp_stride=39),
}
MESH_UNSUPPORTED = {"kv 17": dict(kv=17), "kc 17": dict(kc=17), "5 shift vectors": dict(n_shifts=5)}


def _check(lib, entry, good, bad):
    for what, (mchange, achange) in bad.items():
        m = _mesh(good[0], **mchange)
        args = [ctypes.byref(m)] + list(good[1:])
        for k, v in achange.items():
            args[k] = v
        assert getattr(lib, entry)(*args, None) == L.FG_ERR_INVALID_ARG, what
        assert entry.encode() in lib.fg_last_error(), what
    for what, mchange in MESH_UNSUPPORTED.items():
        m = _mesh(good[0], **mchange)
        assert getattr(lib, entry)(ctypes.byref(m), *good[1:], None) == L.FG_ERR_UNSUPPORTED, what
    assert getattr(lib, entry)(None, *good[1:], None) == L.FG_ERR_INVALID_ARG


@pytest.mark.parametrize("lib_name", ["fp32", "fp64"])
def test_argument_checks_answer_before_any_launch(lib_name):
    lib = L.load() if lib_name == "fp32" else L.load_f64()
    faults = {what: (change, {}) for what, change in MESH_FAULTS.items()}
    # (mesh, points, points_env_stride, n_points, start_cell, max_walk, cell_out, xi_out, status_out)
    bad = {"null points": ({}, {1: None}), "null start_cell": ({}, {4: None}), "null cell_out": ({}, {6: None}), "null xi_out": ({}, {7: None}),
           "null status_out": ({}, {8: None}), "n_points 0": ({}, {3: 0}), "max_walk negative": ({}, {5: -1}), "odd env stride": ({}, {2: 73})}
    _check(lib, "fg_mb_point_locate", [lib_name, ONE, 0, 37, ONE, 256, ONE, ONE, ONE], {**bad, **faults})
    # (mesh, extra, extra_stride, n_extra, cell, xi, cell_env_stride, n_points, out)
    extra, stride = (ctypes.c_void_p * 2)(ONE, ONE), (ctypes.c_int64 * 2)(96, 96)
    bad = {"null cell": ({}, {4: None}), "null xi": ({}, {5: None}), "null out": ({}, {8: None}), "n_points 0": ({}, {7: 0}),
           "n_extra negative": ({}, {3: -1}), "n_extra 9": ({}, {3: 9}), "null extra table": ({}, {1: None}), "null stride table": ({}, {2: None}),
           "null extra field": ({}, {1: (ctypes.c_void_p * 2)(ONE, None)}), "short extra stride": ({}, {2: (ctypes.c_int64 * 2)(96, 95)}),
           "short env stride of the cells": ({}, {6: 36})}
    _check(lib, "fg_mb_point_sample", [lib_name, extra, stride, 2, ONE, ONE, 0, 37, ONE], {**bad, **faults})
    # (mesh, dt, substeps, respawn_slots, seed_pos, seed_cell, pos, cell, age, wraps, lost, n_tracers)
    bad = {"null respawn_slots": ({}, {3: None}), "null seed_pos": ({}, {4: None}), "null seed_cell": ({}, {5: None}), "null pos": ({}, {6: None}),
           "null cell": ({}, {7: None}), "null age": ({}, {8: None}), "null wraps": ({}, {9: None}), "null lost": ({}, {10: None}),
           "substeps 0": ({}, {2: 0}), "substeps negative": ({}, {2: -2}), "n_tracers 0": ({}, {11: 0}), "dt NaN": ({}, {1: float("nan")}),
           "dt infinite": ({}, {1: float("inf")})}
    _check(lib, "fg_mb_tracer_advect", [lib_name, 0.1, 4, ONE, ONE, ONE, ONE, ONE, ONE, ONE, ONE, 64], {**bad, **faults})


def test_refusals_of_the_env_interface():
    from fluidgym_amd.envs.cylinder import CylinderEnvBase, CylinderJetEnv2D
    from fluidgym_amd.envs.airfoil import AirfoilEnvBase
    from fluidgym_amd.envs.parallel_env import ParallelFluidEnv
    from fluidgym_amd.envs.tracers import MeshTracerMixin

    for entry, call in (("locate_probes", lambda: ParallelFluidEnv.locate_probes(None, np.zeros((1, 2)))),
                        ("start_mesh_tracers", lambda: ParallelFluidEnv.start_mesh_tracers(None, 4, seed=0)),
                        ("stop_mesh_tracers", lambda: ParallelFluidEnv.stop_mesh_tracers(None))):
        with pytest.raises(NotImplementedError, match=entry + " is not implemented for ParallelFluidEnv."):
            call()
    assert issubclass(CylinderEnvBase, MeshTracerMixin) and issubclass(AirfoilEnvBase, MeshTracerMixin)
    env = object.__new__(CylinderJetEnv2D)                  # the interface alone: no domain yet
    env._domain = None
    assert env.mesh_tracers is None and env.tracers is None
    for call in (lambda: env.locate_probes(np.zeros((1, 2))), lambda: env.start_mesh_tracers(4, seed=0), env.stop_mesh_tracers):
        with pytest.raises(RuntimeError, match="reset"):
            call()
    dom, T, ref = case("cylinder_2d")
    env._domain = dom                                       # a multi-block domain: the single-block names still refuse, and say where to go
    for call in (lambda: env.probe(np.zeros((1, 2))), lambda: env.start_tracers(4, seed=0), env.stop_tracers):
        with pytest.raises(NotImplementedError, match="single-block.*locate_probes"):
            call()
    with pytest.raises(NotImplementedError, match="multi-block"):
        M.MbPointMesh(object())
    with pytest.raises(ValueError, match="exactly one"):
        M.MeshTracerCloud(object(), 4)
