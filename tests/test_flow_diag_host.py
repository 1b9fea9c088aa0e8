"""Velocity-gradient diagnostics without a GPU: the header, the ctypes signatures and both libraries agree on the two entries and the
five kinds; argument errors answer with status codes before anything touches a device; and the checker the GPU tests use
(``tests/flow_diag_ref.py``) reproduces the rigid-rotation values it is later held against."""
import ctypes
import os
import re

import numpy as np
import pytest

from fluidgym_amd import _lib as L
from oracle import piso_oracle as O
from tests import flow_diag_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("fg_flow_diagnostic", "fg_mb_flow_diagnostic")
KIND_NAMES = ("FG_DIAG_GRADIENT", "FG_DIAG_VORTICITY", "FG_DIAG_VORTICITY_MAGNITUDE", "FG_DIAG_Q", "FG_DIAG_STRAIN_NORM")


def test_header_signatures_and_both_libraries_carry_the_entries_and_kinds():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fluidgym_hip.h")).read(), flags=re.S)
    for k, name in enumerate(KIND_NAMES):
        m = re.search(rf"#define\s+{name}\s+(\d+)", text)
        assert m and int(m.group(1)) == k == getattr(L, name), name
    assert re.search(r"int\s+fg_flow_diagnostic\s*\(\s*fg_handle\s+\w+,\s*int\s+kind,\s*fg_real\s*\*\s*out,\s*void\s*\*\s*stream\s*\)", text)
    assert re.search(r"int\s+fg_mb_flow_diagnostic\s*\(\s*fg_mb_handle\s+\w+,\s*int\s+kind,\s*fg_real\s*\*\s*out,\s*void\s*\*\s*stream\s*\)", text)
    want = (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p])
    for lib, sigs in ((L.load(), L.SIGNATURES), (L.load_f64(), L.SIGNATURES_F64)):
        for name in ENTRIES:
            assert sigs[name] == want, name
            assert hasattr(lib, name), name


def test_channel_counts():
    assert [L.diagnostic_channels(2, k) for k in range(5)] == [4, 1, 1, 1, 1]
    assert [L.diagnostic_channels(3, k) for k in range(5)] == [9, 3, 1, 1, 1]
    assert [R.channels(d, k) for d in (2, 3) for k in R.KINDS] == [L.diagnostic_channels(d, k) for d in (2, 3) for k in range(5)]
    with pytest.raises(ValueError):
        L.diagnostic_channels(2, 5)


@pytest.mark.parametrize("f64", [False, True])
def test_argument_errors_answer_with_status_codes_without_a_launch(f64):
    lib = L.load_f64() if f64 else L.load()
    real, cr = (np.float64, ctypes.c_double) if f64 else (np.float32, ctypes.c_float)
    out = np.full(16, -7.0, real)
    po = ctypes.c_void_p(out.ctypes.data)
    for name in ENTRIES:
        assert getattr(lib, name)(None, L.FG_DIAG_GRADIENT, po, None) == L.FG_ERR_INVALID_ARG
        assert b"null" in lib.fg_last_error()
    # a host-only multi-block handle (device < 0): tables only, nothing computes
    h = ctypes.c_void_p()
    assert lib.fg_mb_create(2, 1, -1, ctypes.byref(h)) == 0
    c = np.ascontiguousarray(np.stack(np.meshgrid(np.linspace(0, 1, 4), np.linspace(0, 1, 5), indexing="xy")), dtype=real)
    bid = ctypes.c_int32(-1)
    assert lib.fg_mb_add_block(h, c.ctypes.data_as(ctypes.POINTER(cr)), 3, 4, 1, ctypes.byref(bid)) == 0
    assert lib.fg_mb_finalize(h) == 0
    assert lib.fg_mb_flow_diagnostic(h, L.FG_DIAG_VORTICITY, None, None) == L.FG_ERR_INVALID_ARG
    assert lib.fg_mb_flow_diagnostic(h, 5, po, None) == L.FG_ERR_INVALID_ARG and b"kind" in lib.fg_last_error()
    assert lib.fg_mb_flow_diagnostic(h, -1, po, None) == L.FG_ERR_INVALID_ARG
    assert lib.fg_mb_flow_diagnostic(h, L.FG_DIAG_VORTICITY, po, None) == L.FG_ERR_UNSUPPORTED
    assert b"host-only" in lib.fg_last_error()
    assert lib.fg_mb_destroy(h) == 0
    assert (out == -7.0).all()


@pytest.mark.parametrize("dims", [2, 3])
def test_checker_reproduces_the_rigid_rotation_on_the_uniform_grid(dims):
    case = R.rigid_single_case(dims)
    grid = case.grid()
    eps = np.finfo(np.float64).eps
    for b, (omega, _) in enumerate(R.RIGID_2D if dims == 2 else R.RIGID_3D):
        dom = case.oracle_domain(b, grid)
        g, A = R.single_block_gradient(dom)
        assert np.array_equal(g, O.velocity_gradient(dom))          # the single-block gradient IS the oracle's
        _check_rigid(g, A, dims, omega, eps)


def test_checker_reproduces_the_rigid_rotation_on_the_affine_two_block_mesh():
    spec, fields = R.rigid_affine_spec()
    dom = spec.oracle()
    M = dom.blocks[0].Minv
    assert np.abs(M[..., 0, 1]).min() > 0.1 and np.abs(M[..., 1, 0]).min() > 0.1      # sheared: Minv is full
    eps = np.finfo(np.float64).eps
    for (u, bv), (omega, _) in zip(fields, R.RIGID_2D):
        R.set_oracle_boundary(dom, bv)
        g, A = R.multi_block_gradient(dom, u)
        _check_rigid(g, A, 2, omega, eps)


def _check_rigid(g, A, dims, omega, eps):
    w_exact, q_exact = R.rigid_expected(dims, omega)
    tol_w, tol_q, tol_s = R.rigid_bounds(A, eps)
    shape = (-1,) + (1,) * (g.ndim - 2)
    w, _ = R.derived(g, R.VORTICITY)
    assert (np.abs(w - w_exact.reshape(shape)) <= tol_w).all()
    assert (np.abs(R.derived(g, R.VORTICITY_MAGNITUDE)[0][0] - np.sqrt((w_exact ** 2).sum())) <= tol_w.sum(axis=0)).all()
    assert (np.abs(R.derived(g, R.Q)[0][0] - q_exact) <= tol_q).all()
    assert (R.derived(g, R.STRAIN_NORM)[0][0] <= tol_s).all()
    assert np.abs(g).max() > 0.4 and (np.abs(g) <= A * (1 + 8 * eps)).all()
