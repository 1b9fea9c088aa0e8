"""Every kernel form of the single-block preconditioners z = M^-1 r against an fp64 reference of the same operator
(tests/precond_reference.py: the oracle's matrices, sparse LU).  The forms are picked at run time by the grid shape and the batch; each
case asserts, through the forms_out of the debug entries, that the branch it was written for is the one that ran.

Pressure (fg_debug_apply_pressure_preconditioner): form 0 = the grid's A = 1 operator (fg_fd_apply), form 1 = the row-mean operator with
factors from k_fd_rowmean_factor, form 2 = the same with the factors made inside the tridiagonal launch (FAC) from the row sums of the
velocity assembly.  Helmholtz (mode 3) and y-line (mode 1): fg_debug_apply_preconditioner."""
import numpy as np
import pytest
import torch

import fluidgym_amd._lib as L
from fluidgym_amd._lib import NativeLibraryError
from fluidgym_amd.simulation.fd_precond import FDPreconditioner
from tests import precond_reference as R
from tests.helpers import make_case

pytestmark = pytest.mark.gpu

TOL = 2e-5          # relative error of z (fp32)
RZ_TOL = 1e-5       # the fused r.z against NumPy
# the row-mean forms make their factors on the device in fp32 (k_fd_rowmean_factor / FAC): the lowest x modes (0 and 1) meet the
# (nearly) singular Neumann operator along y, whose pivots lose accuracy down the rows.  Measured against the fp64 reference: 2.7e-5 ..
# 4.1e-4 at 192 .. 320 rows, the error in modes 0 and 1 (the A = 1 factors, made in fp64 on the host, stay under 2e-5 on the same
# grids).  A dropped or misplaced coefficient is an O(1) error.
ROWMEAN_TOL = 1e-3


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _case(dims, n, fixed_axes, B, uniform_x, seed=3, stretch=0.35, **kw):
    case = make_case(dims=dims, n=n, fixed_axes=fixed_axes, B=B, seed=seed, stretch=stretch, vel_scale=0.3, **kw)
    if uniform_x:
        nx = n[0]
        w = np.full(nx, 2.0 / nx, np.float32)
        case.widths[0] = w
        case.edges[0] = np.concatenate([[0.0], np.cumsum(w.astype(np.float64))])
    return case


def _envs(B):
    """a seeded subset of a large batch: the first, the last and one in the middle"""
    return sorted({0, B // 2, B - 1})


def _inputs(case, seed=7):
    rng = np.random.default_rng(seed)
    r = rng.standard_normal((case.B,) + case.shape)
    r -= r.mean(axis=tuple(range(1, r.ndim)), keepdims=True)
    # a different 1/A per env, varying along x and across the rows (a mix-up between envs or rows shows)
    rA = rng.uniform(0.6, 1.4, size=(case.B,) + case.shape) * (1.0 + np.arange(case.B)).reshape((-1,) + (1,) * len(case.shape))
    return r.astype(np.float32), (rA / 100.0).astype(np.float32)


def _check_pressure(ns, case, form, r, rA_np, expect, rA_dev=None):
    g = case.grid()
    z, rz, forms = ns.apply_pressure_preconditioner(form, torch.from_numpy(r).cuda(), rA_dev)
    torch.cuda.synchronize()
    for slot, code in expect.items():
        assert forms[slot] == code, (form, forms, expect)
    zz = _np(z)
    for b in _envs(case.B):
        A = 1.0 if form == 0 else R.rowmean_A(rA_np[b].astype(np.float64))
        ref = R.solve_pressure(R.pressure_operator(case, g, A), r[b])
        got = zz[b] - zz[b].mean()
        assert R.rel_err(got, ref) < (TOL if form == 0 else ROWMEAN_TOL), (form, b, R.rel_err(got, ref))
        dot = float(np.dot(r[b].astype(np.float64).ravel(), zz[b].ravel()))
        assert abs(rz[b] - dot) <= RZ_TOL * max(abs(dot), 1e-30), (form, b, rz[b], dot)
    return forms


# ---------------------------------------------------------------------------------------------------------------------------
# pressure, x bases and GEMM tiles (form 0; the row-mean forms where the grid carries them)
X = L.FG_FORM_SLOT_X
Z = L.FG_FORM_SLOT_Z
TRI = L.FG_FORM_SLOT_TRIDIAG
FAC = L.FG_FORM_SLOT_FACTORS

BASES = [
    # (dims, n, fixed_axes, B, uniform x, expected forms of form 0)
    (2, (64, 24), (0, 1), 3, True, {X: L.FG_FORM_DCT, TRI: L.FG_FORM_TRI_LDS3}),
    (2, (128, 40), (0, 1), 3, True, {X: L.FG_FORM_DCT}),
    (2, (256, 19), (0, 1), 3, True, {X: L.FG_FORM_DCT}),
    (2, (512, 16), (0, 1), 3, True, {X: L.FG_FORM_DCT}),
    (2, (128, 33), (1,), 3, True, {X: L.FG_FORM_FFT}),
    (2, (60, 24), (0, 1), 3, False, {X: L.FG_FORM_GEMM_SPLITK, TRI: L.FG_FORM_TRI_LDS3}),
    (2, (96, 20), (1,), 4, False, {X: L.FG_FORM_GEMM_SPLITK}),
    (3, (20, 9, 6), (1,), 3, False, {X: L.FG_FORM_GEMM_SPLITK, Z: L.FG_FORM_GEMM_SPLITK, TRI: L.FG_FORM_TRI_LDS3}),
    (2, (192, 256), (0, 1), 32, False, {X: L.FG_FORM_GEMM_T64, TRI: L.FG_FORM_TRI_LDS2}),
]


@pytest.mark.parametrize("dims,n,fixed_axes,B,uniform_x,expect", BASES)
def test_pressure_preconditioner_bases_and_gemm_tiles(dims, n, fixed_axes, B, uniform_x, expect):
    case = _case(dims, n, fixed_axes, B, uniform_x)
    ns = case.native()
    r, rA = _inputs(case)
    _check_pressure(ns, case, 0, r, rA, {**expect, FAC: L.FG_FORM_FAC_GRID})
    rowmean = dims == 2 and uniform_x and n[0] % 64 == 0 and n[1] <= 320
    if rowmean:
        _check_pressure(ns, case, 1, r, rA, {FAC: L.FG_FORM_FAC_ROWMEAN, X: expect[X]}, torch.from_numpy(rA).cuda())
    else:
        with pytest.raises(NativeLibraryError, match=r"status -4"):
            ns.apply_pressure_preconditioner(1, torch.from_numpy(r).cuda(), torch.from_numpy(rA).cuda())
    ns.close()


def test_pressure_preconditioner_128_and_z64_tiles_in_3d():
    """3-D stretched x 128 x 64 x 64, B = 16: the x basis change takes the 128 x 128 tile (32 row tiles x 16 envs = 512 big blocks), the
    z basis change the 64 x 128 tile with the whole K (M = K = 64).  Too large for a sparse factorisation: the reference is the NumPy
    application of the same factors (tests/test_precond_reference.py shows it equals the oracle solve on small grids)."""
    case = _case(3, (128, 64, 64), (1,), 16, False, stretch=0.3)
    ns = case.native()
    r, _ = _inputs(case)
    z, rz, forms = ns.apply_pressure_preconditioner(0, torch.from_numpy(r).cuda())
    torch.cuda.synchronize()
    assert forms[X] == L.FG_FORM_GEMM_T128 and forms[Z] == L.FG_FORM_GEMM_Z64, forms
    assert forms[TRI] == L.FG_FORM_TRI_LDS3 and forms[FAC] == L.FG_FORM_FAC_GRID, forms
    fd = FDPreconditioner(case.widths, case.fixed_faces)
    zz = _np(z)
    for b in _envs(case.B):
        ref = fd.apply(r[b].astype(np.float64))
        assert R.rel_err(zz[b] - zz[b].mean(), ref - ref.mean()) < TOL, b
        dot = float(np.dot(r[b].astype(np.float64).ravel(), zz[b].ravel()))
        assert abs(rz[b] - dot) <= RZ_TOL * abs(dot)
    ns.close()


# ---------------------------------------------------------------------------------------------------------------------------
# pressure, tridiagonal forms and the row-mean / FAC edges: all three forms; form 2 needs the row sums of a velocity assembly
EDGES = [
    # (n, fixed_axes, B, form 0 tridiagonal, form 2 tridiagonal or None = refused)
    ((64, 192), (0, 1), 3, L.FG_FORM_TRI_LDS3, L.FG_FORM_TRI_LDS3_FAC),
    ((64, 193), (0, 1), 3, L.FG_FORM_TRI_LDS3, L.FG_FORM_TRI_LDS2_FAC),
    ((64, 208), (0, 1), 3, L.FG_FORM_TRI_LDS3, L.FG_FORM_TRI_LDS2_FAC),
    ((64, 209), (0, 1), 3, L.FG_FORM_TRI_LDS2, L.FG_FORM_TRI_LDS2_FAC),
    ((64, 304), (0, 1), 3, L.FG_FORM_TRI_LDS2, L.FG_FORM_TRI_LDS2_FAC),
    ((64, 305), (0, 1), 3, L.FG_FORM_TRI_LDS2, None),
    ((64, 320), (0, 1), 3, L.FG_FORM_TRI_LDS2, None),
    ((64, 321), (0, 1), 3, L.FG_FORM_TRI_STREAM, None),
    ((256, 128), (0, 1), 64, L.FG_FORM_TRI_LDS3, L.FG_FORM_TRI_LDS3_FAC),     # the headline grid and batch
]


@pytest.mark.parametrize("n,fixed_axes,B,tri0,tri2", EDGES)
def test_pressure_preconditioner_tridiagonal_forms_and_rowmean_edges(n, fixed_axes, B, tri0, tri2):
    case = _case(2, n, fixed_axes, B, True, through_flow_axis=0)
    ns = case.native()
    r, rA = _inputs(case)
    _check_pressure(ns, case, 0, r, rA, {X: L.FG_FORM_DCT, TRI: tri0, FAC: L.FG_FORM_FAC_GRID})
    rowmean = n[1] <= 320
    if rowmean:
        # form 1 runs the same tridiagonal kernel as form 0, with the env's own factors
        _check_pressure(ns, case, 1, r, rA, {X: L.FG_FORM_DCT, TRI: tri0, FAC: L.FG_FORM_FAC_ROWMEAN}, torch.from_numpy(rA).cuda())
    else:
        with pytest.raises(NativeLibraryError, match=r"status -4"):
            ns.apply_pressure_preconditioner(1, torch.from_numpy(r).cuda(), torch.from_numpy(rA).cuda())
    ns.setup_advection([0.02 + 0.01 * (b % 3) for b in range(B)])
    rA_asm = (1.0 / ns.buffer(L.FG_BUF_A, (B,) + case.shape)).cpu().numpy()
    if tri2 is None:
        with pytest.raises(NativeLibraryError, match=r"status -4"):
            ns.apply_pressure_preconditioner(2, torch.from_numpy(r).cuda())
    else:
        _check_pressure(ns, case, 2, r, rA_asm, {X: L.FG_FORM_DCT, TRI: tri2, FAC: L.FG_FORM_FAC_MADE})
    ns.close()


@pytest.mark.parametrize("n", [(30, 40), (30, 300)])
def test_pressure_preconditioner_streaming_tridiagonal_for_rows_not_a_multiple_of_four(n):
    """nx % 4 != 0: the streaming k_tridiag_y.  At 300 rows its y buffer (320 x 64 floats, 80 KB) needs the dynamic-LDS opt-in."""
    case = _case(2, n, (0, 1), 3, False)
    ns = case.native()
    r, rA = _inputs(case)
    _check_pressure(ns, case, 0, r, rA, {X: L.FG_FORM_GEMM_SPLITK, TRI: L.FG_FORM_TRI_STREAM, FAC: L.FG_FORM_FAC_GRID})
    ns.close()


def test_grid_beyond_the_tridiagonal_lds_is_refused_when_the_solver_is_built():
    """More than 640 rows: the streaming tridiagonal kernel cannot hold the column in LDS.  The FD preconditioner is refused when the
    solver is built (plain CG is the pressure solver), never inside a solve."""
    case = _case(2, (30, 700), (0, 1), 2, False)
    ns = case.native()
    assert not ns.has_fd and ns.default_method == L.FG_SOLVER_CG
    r, _ = _inputs(case)
    with pytest.raises(NativeLibraryError, match=r"status -1: .*fg_set_fd_preconditioner was not called"):
        ns.apply_pressure_preconditioner(0, torch.from_numpy(r).cuda())
    ns.close()


def test_pressure_preconditioner_fp64_build():
    """The fp64 library carries form 0 (fg_f64_fd.hip: the same factors, applied in doubles): against the NumPy application of those
    factors at 1e-12; the row-mean forms are refused."""
    case = _case(2, (24, 16), (1,), 3, False)
    ns = case.native(dtype=torch.float64)
    r, rA = _inputs(case)
    r = r.astype(np.float64)
    z, rz, forms = ns.apply_pressure_preconditioner(0, torch.from_numpy(r).cuda())
    torch.cuda.synchronize()
    assert forms[X] == L.FG_FORM_F64 and forms[TRI] == L.FG_FORM_TRI_F64, forms
    fd = FDPreconditioner(case.widths, case.fixed_faces)
    zz = _np(z)
    for b in range(case.B):
        ref = fd.apply(r[b])
        assert R.rel_err(zz[b], ref) < 1e-12, b
        dot = float(np.dot(r[b].ravel(), zz[b].ravel()))
        assert abs(rz[b] - dot) <= 1e-12 * abs(dot)
    for form in (1, 2):
        with pytest.raises(NativeLibraryError, match=r"status -4"):
            ns.apply_pressure_preconditioner(form, torch.from_numpy(r).cuda(), torch.from_numpy(rA.astype(np.float64)).cuda())
    ns.close()


# ---------------------------------------------------------------------------------------------------------------------------
# Helmholtz operator (mode 3): the row form where the BiCGStab runs it, the array form elsewhere
HELM = [
    (2, (64, 32), L.FG_FORM_HELM_ROW32),
    (2, (256, 256), L.FG_FORM_HELM_ROW32),
    (2, (96, 48), L.FG_FORM_HELM_ARRAY),
    (2, (64, 257), L.FG_FORM_HELM_ARRAY),
    (3, (32, 24, 16), L.FG_FORM_HELM_ARRAY),
]


@pytest.mark.parametrize("dims,n,helm", HELM)
def test_helmholtz_preconditioner_forms(dims, n, helm):
    case = _case(dims, n, (1,), 3, False, stretch=0.0, nu=0.05)
    w = (np.linspace(1.0, 3.0, n[1]) ** 1.5).astype(np.float32)       # stretched y: the transform axes stay uniform
    case.widths[1] = (w / w.sum()).astype(np.float32)
    case.edges[1] = np.concatenate([[0.0], np.cumsum(case.widths[1].astype(np.float64))])
    ns = case.native()
    assert ns.has_helmholtz
    dt = [0.02, 0.05, 0.03]
    ns.setup_advection(dt)
    rng = np.random.default_rng(9)
    r = rng.standard_normal((case.B, dims) + case.shape).astype(np.float32)
    z, forms = ns.apply_advection_preconditioner(3, torch.from_numpy(r).cuda(), return_forms=True)
    torch.cuda.synchronize()
    assert forms[L.FG_FORM_SLOT_HELM] == helm, forms
    if helm == L.FG_FORM_HELM_ARRAY:
        assert forms[L.FG_FORM_SLOT_LINE] in (L.FG_FORM_LINE_LDS, L.FG_FORM_LINE_STREAM), forms
    zz = _np(z).reshape(case.B, dims, -1)
    g = case.grid()
    for b in range(case.B):
        ref = R.solve(R.helmholtz_operator(case, b, g, dt[b]), r[b].reshape(dims, -1))
        assert R.rel_err(zz[b], ref) < TOL, (b, R.rel_err(zz[b], ref))
    ns.close()


# ---------------------------------------------------------------------------------------------------------------------------
# y-line solve (mode 1): LDS column block or streaming
LINE = [
    (2, (64, 208), (1,), L.FG_FORM_LINE_LDS),
    (2, (64, 209), (1,), L.FG_FORM_LINE_STREAM),
    (2, (30, 40), (1,), L.FG_FORM_LINE_STREAM),
    (3, (16, 12, 8), (1,), L.FG_FORM_LINE_LDS),
    (2, (32, 24), (0,), L.FG_FORM_LINE_LDS),        # periodic y: no wrap in the line operator
]


@pytest.mark.parametrize("dims,n,fixed_axes,line", LINE)
def test_yline_preconditioner_forms(dims, n, fixed_axes, line):
    case = _case(dims, n, fixed_axes, 3, False, seed=5)
    ns = case.native()
    dt = 0.04
    ns.setup_advection(dt)
    rng = np.random.default_rng(3)
    r = rng.standard_normal((case.B, dims) + case.shape).astype(np.float32)
    z, forms = ns.apply_advection_preconditioner(1, torch.from_numpy(r).cuda(), return_forms=True)
    torch.cuda.synchronize()
    assert forms[L.FG_FORM_SLOT_LINE] == line, forms
    zz = _np(z).reshape(case.B, dims, -1)
    g = case.grid()
    from oracle import piso_oracle as O
    for b in range(case.B):
        C, _, _ = O.build_advection_matrix(case.oracle_domain(b, g), dt)
        ref = R.solve(R.yline_operator(C, case.shape), r[b].reshape(dims, -1))
        assert R.rel_err(zz[b], ref) < TOL, (b, R.rel_err(zz[b], ref))
    ns.close()
