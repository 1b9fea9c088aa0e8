"""CPU-side checks of the point probes and tracers (``fluidgym_amd/simulation/tracers.py``, ``csrc/fg_tracers.hip``; DESIGN.md section
6p).  Part 1 holds the NumPy restatement the GPU tests compare against (``tests/tracers_ref.py``) to analytic facts, and the host
helpers to their contracts; part 2 holds the two entry points to their argument checks, which answer before any launch."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from fluidgym_amd import _lib as L
from fluidgym_amd.envs.parallel_env import ParallelFluidEnv
from fluidgym_amd.simulation import tracers as TR
from tests import tracers_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fg_point_sample", "fg_tracer_advect")


def _stretched(n, lo, hi, ratio=1.3):
    h = ratio ** np.arange(n)
    return lo + (hi - lo) * np.concatenate([[0.0], np.cumsum(h) / h.sum()])


def _affine_case(dims, periodic, rng):
    """A grid with a stretched y, an affine velocity sampled at the centres and on the FIXED faces, an affine scalar."""
    edges = [np.linspace(-1.0, 2.0, 9), _stretched(6, 0.5, 2.0), np.linspace(0.0, 1.0, 5)][:dims]
    grid = R.RefGrid.from_edges(edges, periodic)
    A, b = rng.standard_normal((dims, dims)), rng.standard_normal(dims)
    centres = [0.5 * (e[1:] + e[:-1]) for e in edges]

    def field(axes_coords):              # [d, (Z,) Y, X] of A x + b on the product of per-axis coordinates
        mesh = np.meshgrid(*reversed(axes_coords), indexing="ij")[::-1]          # x, y(, z) arrays of shape [(Z,) Y, X]
        return np.stack([sum(A[c, a] * mesh[a] for a in range(dims)) + b[c] for c in range(dims)])

    bvel = {}
    for a in range(dims):
        if not periodic[a]:
            for side in (0, 1):
                coords = list(centres)
                coords[a] = np.array([edges[a][-1 if side else 0]])
                bvel[2 * a + side] = field(coords)
    return edges, grid, A, b, field(centres), bvel


# ------------------------------------------------------------------------------------------------ part 1: the restatement
@pytest.mark.parametrize("dims,periodic", [(2, (False, False)), (2, (True, False)), (3, (True, False, True)), (3, (False, False, False))])
def test_reference_reproduces_affine_fields(dims, periodic):
    rng = np.random.default_rng(dims * 10 + sum(periodic))
    edges, grid, A, b, vel, bvel = _affine_case(dims, periodic, rng)
    # interior points: anywhere along a FIXED axis (the faces carry affine values), between the first and the last centre along a
    # periodic one (an affine field is not periodic: the seam interval cannot reproduce it)
    # (and one FIXED axis at a time: in an edge cell of the box, where a corner is a face node on two axes, the face array is read at
    # the adjacent cell's index, which is constant extrapolation along the other axis)
    first, last = np.array([0.5 * (e[0] + e[1]) for e in edges]), np.array([0.5 * (e[-2] + e[-1]) for e in edges])
    sets = []
    for a in [a for a in range(dims) if not periodic[a]]:
        lo, hi = first.copy(), last.copy()
        lo[a], hi[a] = edges[a][0], edges[a][-1]
        sets.append(lo + rng.random((100, dims)) * (hi - lo))
    pts = np.concatenate(sets)
    pts[:4, 1] = edges[1][0] + 1e-3 * rng.random(4)                      # between the wall and the first centre
    got = R.sample_velocity(grid, vel, bvel, pts)
    assert np.abs(got - (pts @ A.T + b)).max() < 1e-13
    scal = vel[0]                                                        # an affine scalar: reproduced away from the faces only
    inner = np.all((pts >= [0.5 * (e[0] + e[1]) for e in edges]) & (pts <= [0.5 * (e[-2] + e[-1]) for e in edges]), axis=1)
    assert inner.sum() > 20
    assert np.abs(R.sample_scalar(grid, scal, pts[inner]) - (pts[inner] @ A[0] + b[0])).max() < 1e-13
    # at a node the value is the node's, bit for bit
    cx, cy = 0.5 * (edges[0][2] + edges[0][3]), 0.5 * (edges[1][4] + edges[1][5])
    p = np.array([[cx, cy] + ([0.5 * (edges[2][1] + edges[2][2])] if dims == 3 else [])])
    assert np.array_equal(R.sample_velocity(grid, vel, bvel, p)[0], vel[(slice(None),) + ((1,) if dims == 3 else ()) + (4, 2)])
    p[0, 1] = edges[1][-1]
    assert np.array_equal(R.sample_velocity(grid, vel, bvel, p)[0], bvel[3][(slice(None),) + ((1,) if dims == 3 else ()) + (0, 2)])


def test_reference_constant_field_across_the_seam_and_corner_rule():
    edges = [np.linspace(0.0, 4.0, 9), _stretched(6, 0.0, 1.0)]
    grid = R.RefGrid.from_edges(edges, (True, False))
    vel = np.full((2, 6, 8), 0.75)
    bvel = {2: np.full((2, 1, 8), 0.75), 3: np.full((2, 1, 8), 0.75)}
    pts = np.array([[0.01, 0.3], [3.99, 0.9], [4.0, 0.5], [-0.2, 0.5], [7.9, 0.2]])
    assert np.array_equal(R.sample_velocity(grid, vel, bvel, pts), np.full((5, 2), 0.75))
    # the seam interval blends the last and the first column
    vel = np.tile(np.arange(8.0), (2, 6, 1))
    got = R.sample_velocity(grid, vel, {2: vel[:, :1], 3: vel[:, :1]}, np.array([[0.0, 0.5]]))
    assert np.allclose(got, 3.5, atol=1e-14)
    # a corner of an all-FIXED box reads the y face (the order y, x, z)
    g2 = R.RefGrid.from_edges(edges, (False, False))
    bv = {0: np.full((2, 6, 1), 10.0), 1: np.full((2, 6, 1), 11.0), 2: np.full((2, 1, 8), 12.0), 3: np.full((2, 1, 8), 13.0)}
    z = np.zeros((2, 6, 8))
    assert np.array_equal(R.sample_velocity(g2, z, bv, np.array([[0.0, 0.0], [4.0, 1.0], [0.0, 0.5]])), [[12, 12], [13, 13], [10, 10]])
    # a NaN position lands in a valid interval and gives a NaN, without an index error
    assert np.isnan(R.sample_velocity(g2, z, bv, np.array([[np.nan, 0.5]]))).all()


def test_reference_midpoint_step_of_a_solid_body_rotation():
    """u = -W y, v = W x: one midpoint step is (I + h A + h^2 A^2 / 2) x."""
    W, h = 0.7, 0.05
    edges = [np.linspace(-1.0, 1.0, 9), _stretched(6, -1.0, 1.0, 1.2)]
    grid = R.RefGrid.from_edges(edges, (False, False))
    A = np.array([[0.0, -W], [W, 0.0]])
    c = [0.5 * (e[1:] + e[:-1]) for e in edges]
    f = lambda x, y: np.stack([-W * y + 0 * x, W * x + 0 * y])
    vel = f(c[0][None, :], c[1][:, None])
    bvel = {0: f(edges[0][:1][None, :], c[1][:, None]), 1: f(edges[0][-1:][None, :], c[1][:, None]),
            2: f(c[0][None, :], edges[1][:1][:, None]), 3: f(c[0][None, :], edges[1][-1:][:, None])}
    x0 = np.random.default_rng(1).uniform(-0.6, 0.6, (50, 2))
    x1, age, wraps, lost = R.advect(grid, vel, bvel, x0, x0, np.zeros(50), np.zeros((50, 2), np.int64), h, 1)
    assert np.abs(x1 - x0 @ (np.eye(2) + h * A + 0.5 * h * h * A @ A).T).max() < 1e-14
    assert lost == 0 and not wraps.any() and np.array_equal(age, np.full(50, h))
    # four sub-steps of h / 4 are the fourth power of the sub-step's map
    x4, *_ = R.advect(grid, vel, bvel, x0, x0, np.zeros(50), np.zeros((50, 2), np.int64), h, 4)
    M = np.eye(2) + (h / 4) * A + 0.5 * (h / 4) ** 2 * A @ A
    assert np.abs(x4 - x0 @ np.linalg.matrix_power(M, 4).T).max() < 1e-14


def test_reference_wrap_respawn_and_clamp():
    edges = [np.linspace(0.0, 2.0, 9), np.linspace(0.0, 1.0, 7)]
    grid = R.RefGrid.from_edges(edges, (True, False))
    vel = np.stack([np.full((6, 8), 3.0), np.full((6, 8), -2.0)])
    bvel = {2: vel[:, :1].copy(), 3: vel[:, :1].copy()}
    seed = np.array([[1.5, 0.9], [0.1, 0.05]])
    pos, age, wraps, lost = R.advect(grid, vel, bvel, seed, seed, np.zeros(2), np.zeros((2, 2), np.int64), 0.25, 2)
    assert np.allclose(pos, [[0.25, 0.4], [0.85, 0.0]]) and wraps.tolist() == [[1, 0], [0, 0]] and lost == 0      # wrapped; clamped
    pos, age, wraps, lost = R.advect(grid, vel, bvel, seed, seed, np.ones(2), np.zeros((2, 2), np.int64), 0.25, 2, respawn_faces=1 << 2)
    assert np.array_equal(pos[1], seed[1]) and age.tolist() == [1.25, 0.0]                                        # respawned at its seed
    x, k = R.wrap(np.array([-0.5, 2.0, 4.5, 1.0]), 0.0, 2.0)
    assert np.array_equal(x, [1.5, 0.0, 0.5, 1.0]) and k.tolist() == [-1, 1, 2, 0]


def test_seeds_do_not_depend_on_the_batch_size():
    lo, length = np.array([0.0, -1.0, 2.0]), np.array([4.0, 2.0, 1.0])
    a, b = TR.seed_positions(5, 2, 64, lo, length), TR.seed_positions(5, 5, 64, lo, length)
    assert a.shape == (2, 64, 3) and b.shape == (5, 64, 3) and a.dtype == np.float64
    assert np.array_equal(a, b[:2]) and not np.array_equal(b[0], b[1])
    assert np.array_equal(a[1], lo + np.random.default_rng([5, 1]).random((64, 3)) * length)                     # the recorded draw order
    assert (a >= lo).all() and (a < lo + length).all()
    assert not np.array_equal(TR.seed_positions(6, 2, 64, lo, length), a)
    # the node arrays of the host side are those of the restatement, rounded
    edges = [np.linspace(0.0, 4.0, 9), _stretched(6, -1.0, 1.0)]
    for dtype in (np.float32, np.float64):
        mine = TR.node_arrays(edges, (True, False), dtype)
        ref = R.RefGrid.from_edges(edges, (True, False), dtype)
        for a_, (nodes, lo_, len_) in enumerate(mine):
            assert nodes.dtype == dtype and np.array_equal(nodes, ref.nodes[a_]) and lo_ == ref.lo[a_] and len_ == ref.len[a_]
        assert len(mine[0][0]) == 8 and len(mine[1][0]) == 8


def test_host_refusals():
    with pytest.raises(NotImplementedError, match="single-block"):
        TR.TracerCloud(object(), 4, seed=0)
    with pytest.raises(NotImplementedError, match="single-block"):
        TR.sample_points(object(), np.zeros((3, 2)))
    assert TR.respawn_mask(("-x", "+x"), 2, (False, False)) == 3 and TR.respawn_mask((3,), 3, (True, False, True)) == 8
    with pytest.raises(ValueError, match="periodic"):
        TR.respawn_mask(("-x",), 2, (True, False))
    with pytest.raises(ValueError, match="does not exist"):
        TR.respawn_mask(("-z",), 2, (False, False))
    for entry, call in (("probe", lambda: ParallelFluidEnv.probe(None, np.zeros((1, 2)))),
                        ("start_tracers", lambda: ParallelFluidEnv.start_tracers(None, 4, seed=0)),
                        ("stop_tracers", lambda: ParallelFluidEnv.stop_tracers(None))):
        with pytest.raises(NotImplementedError, match=entry + " is not implemented for ParallelFluidEnv."):
            call()
    import fluidgym_amd

    env = fluidgym_amd.make("RBC2D-easy-v0", cuda_device=torch.device("cpu"))
    assert env.tracers is None
    for call in (lambda: env.probe(np.zeros((1, 2))), lambda: env.start_tracers(4, seed=0), env.stop_tracers):
        with pytest.raises(RuntimeError, match="reset"):
            call()


# ------------------------------------------------------------------------------------------------ part 2: the library
def test_both_libraries_export_the_entry_points():
    header = open(os.path.join(ROOT, "include", "fluidgym_hip.h")).read()
    mk = open(os.path.join(ROOT, "fluidgym_amd", "csrc", "Makefile")).read()
    assert all("fg_tracers.hip" in line for line in mk.splitlines() if line.startswith(("SRCS =", "F64_SRCS =")))
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header)
        assert name in L.SIGNATURES and name in L.SIGNATURES_F64
        assert hasattr(L.load(), name) and hasattr(L.load_f64(), name)
    import fluidgym_amd

    assert fluidgym_amd.TracerCloud is TR.TracerCloud and fluidgym_amd.sample_points is TR.sample_points and fluidgym_amd.PointGrid is TR.PointGrid
    body = re.search(r"typedef struct fg_point_grid \{(.*?)\} fg_point_grid;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        if decl.strip():
            names += [re.match(r"\W*(\w+)", x).group(1) for x in decl.strip().rsplit("*", 1)[-1].split(None, 1)[-1].split(",")]
    assert names == [f[0] for f in L.FgPointGrid._fields_] == [f[0] for f in L.FgPointGridF64._fields_]
    assert dict(L.FgPointGridF64._fields_)["lo"]._type_ is ctypes.c_double and dict(L.FgPointGrid._fields_)["lo"]._type_ is ctypes.c_float
    assert L.SIGNATURES_F64["fg_tracer_advect"][1][1] is ctypes.c_double


ONE = 4096                  # a "device pointer" that is never dereferenced: every call below fails its argument checks first


def _grid(lib_name, d=2, **change):
    g = (L.FgPointGrid if lib_name == "fp32" else L.FgPointGridF64)()
    dims = d
    g.dims, g.batch, g.nx, g.ny, g.nz = dims, 2, 8, 6, 4 if dims == 3 else 1
    cells = g.nx * g.ny * g.nz
    for a in range(dims):
        g.periodic[a] = int(a != 1)                  # periodic x (and z), FIXED y
        g.nodes[a] = ONE
        g.lo[a], g.len[a] = 0.0, 1.0
    g.velocity, g.velocity_stride = ONE, dims * cells
    for f in (2, 3):
        g.bvel[f], g.bvel_stride[f] = ONE, dims * cells // g.ny
    for k, v in change.items():
        if isinstance(v, tuple):
            getattr(g, k)[v[0]] = v[1]
        else:
            setattr(g, k, v)
    return g


GRID_FAULTS = {
    "dims 1": dict(dims=1), "dims 4": dict(dims=4), "batch 0": dict(batch=0), "batch above 65535": dict(batch=65536),
    "nx 0": dict(nx=0), "ny negative": dict(ny=-3), "nz 0": dict(nz=0), "null velocity": dict(velocity=None),
    "null nodes": dict(nodes=(1, None)), "missing bvel on the FIXED axis": dict(bvel=(3, None)), "short velocity stride": dict(velocity_stride=95),
    "short boundary stride": dict(bvel_stride=(2, 15)), "len 0": dict(len=(0, 0.0)), "len NaN": dict(len=(1, float("nan"))),
    "lo infinite": dict(lo=(0, float("inf"))), "periodic flag 2": dict(periodic=(0, 2)),
}


@pytest.mark.parametrize("lib_name", ["fp32", "fp64"])
def test_point_sample_argument_checks_answer_before_any_launch(lib_name):
    lib = L.load() if lib_name == "fp32" else L.load_f64()
    extra, stride = (ctypes.c_void_p * 2)(ONE, ONE), (ctypes.c_int64 * 2)(48, 48)
    # (grid, extra, extra_stride, n_extra, points, points_env_stride, n_points, out)
    good = [None, extra, stride, 2, ONE, 0, 37, ONE]
    bad = {"null grid": ({}, {0: None}), "null points": ({}, {4: None}), "null out": ({}, {7: None}), "n_points 0": ({}, {6: 0}),
           "n_extra negative": ({}, {3: -1}), "n_extra 9": ({}, {3: 9}), "null extra table": ({}, {1: None}), "null stride table": ({}, {2: None}),
           "null extra field": ({}, {1: (ctypes.c_void_p * 2)(ONE, None)}), "short extra stride": ({}, {2: (ctypes.c_int64 * 2)(48, 47)}),
           "short env stride of the points": ({}, {5: 73})}
    bad.update({what: (change, {}) for what, change in GRID_FAULTS.items()})
    for what, (gchange, achange) in bad.items():
        g = _grid(lib_name, **gchange)
        args = [ctypes.byref(g)] + good[1:]
        for k, v in achange.items():
            args[k] = v
        assert lib.fg_point_sample(*args, None) == L.FG_ERR_INVALID_ARG, what
        assert b"fg_point_sample" in lib.fg_last_error(), what
    g3 = _grid(lib_name, d=3, bvel=(2, None))
    assert lib.fg_point_sample(ctypes.byref(g3), extra, stride, 0, ONE, 0, 37, ONE, None) == L.FG_ERR_INVALID_ARG
    g2 = _grid(lib_name, nz=2)                                                                    # nz must be 1 on a 2-D grid
    assert lib.fg_point_sample(ctypes.byref(g2), extra, stride, 0, ONE, 0, 37, ONE, None) == L.FG_ERR_INVALID_ARG


@pytest.mark.parametrize("lib_name", ["fp32", "fp64"])
def test_tracer_advect_argument_checks_answer_before_any_launch(lib_name):
    lib = L.load() if lib_name == "fp32" else L.load_f64()
    # (grid, dt, substeps, respawn_faces, seed_pos, pos, age, wraps, lost, n_tracers)
    good = [None, 0.1, 4, 0, ONE, ONE, ONE, ONE, ONE, 64]
    bad = {"null grid": ({}, {0: None}), "null seed_pos": ({}, {4: None}), "null pos": ({}, {5: None}), "null age": ({}, {6: None}),
           "null wraps": ({}, {7: None}), "null lost": ({}, {8: None}), "substeps 0": ({}, {2: 0}), "substeps negative": ({}, {2: -2}),
           "n_tracers 0": ({}, {9: 0}), "a respawn bit of a z face in 2-D": ({}, {3: 1 << 4}), "dt NaN": ({}, {1: float("nan")})}
    bad.update({what: (change, {}) for what, change in GRID_FAULTS.items()})
    for what, (gchange, achange) in bad.items():
        g = _grid(lib_name, **gchange)
        args = [ctypes.byref(g)] + good[1:]
        for k, v in achange.items():
            args[k] = v
        assert lib.fg_tracer_advect(*args, None) == L.FG_ERR_INVALID_ARG, what
        assert b"fg_tracer_advect" in lib.fg_last_error(), what
