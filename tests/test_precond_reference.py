"""CPU self-checks of the fp64 preconditioner references in tests/precond_reference.py (the yardsticks of
tests/test_gpu_precond_forms.py): each reference solves the operator it claims to, on small grids."""
import numpy as np
import pytest
import scipy.sparse as sp

from fluidgym_amd.simulation.fd_precond import FDPreconditioner
from oracle import piso_oracle as O
from tests import precond_reference as R
from tests.helpers import make_case


@pytest.mark.parametrize("dims,n,fixed_axes", [(2, (12, 9), (1,)), (2, (10, 7), (0, 1)), (3, (8, 6, 5), (1,)), (3, (7, 6, 4), (0, 1, 2))])
def test_pressure_reference_solves_the_oracle_operator_and_equals_the_fd_factors(dims, n, fixed_axes):
    case = make_case(dims=dims, n=n, fixed_axes=fixed_axes, B=1, seed=3, stretch=0.4)
    g = case.grid()
    P = R.pressure_operator(case, g, 1.0)
    r = np.random.default_rng(1).standard_normal(case.shape)
    x = R.solve_pressure(P, r)
    rr = r - r.mean()
    assert np.abs(P @ x.ravel() - rr.ravel()).max() < 1e-10 * np.abs(rr).max()
    assert abs(x.mean()) < 1e-12 * np.abs(x).max()
    # the NumPy application of the device's factors (float32-stored eigenvectors and pivots, applied in float64) is the same operator,
    # to the float32 rounding of its factors: the reference for the grids too large for a sparse factorisation
    fd = FDPreconditioner(case.widths, case.fixed_faces)
    z = fd.apply(rr)
    assert R.rel_err(z - z.mean(), x) < 2e-6


def test_rowmean_operator_is_the_oracle_matrix_of_the_row_constant_coefficient():
    """Row-mean A: every face coefficient of the oracle matrix equals the device's c_{j+1/2} = (a_j / hy_j + a_{j+1} / hy_{j+1}) / 2
    along y and a_j / hx along x (uniform x), with a_j the row mean of 1/A."""
    case = make_case(dims=2, n=(16, 10), fixed_axes=(0, 1), B=1, seed=2, stretch=0.3)
    g = case.grid()
    rA = np.random.default_rng(4).uniform(0.5, 1.5, size=case.shape)
    A = R.rowmean_A(rA)
    a = rA.mean(axis=1)
    assert np.allclose(1.0 / A, a[:, None], rtol=1e-14)
    _, _, offs = O.build_pressure_matrix(case.oracle_domain(0, g), A)
    hx = case.widths[0].astype(np.float64)
    hy = case.widths[1].astype(np.float64)
    ny, nx = case.shape
    # +y face of row j (face 3) between rows j and j + 1; alpha_y = hx / hy on a rectilinear grid
    for j in range(ny - 1):
        c = 0.5 * (a[j] / hy[j] + a[j + 1] / hy[j + 1]) * hx
        assert np.allclose(offs[3][j], c, rtol=1e-12)
    assert np.allclose(offs[3][ny - 1], 0.0)


def test_helmholtz_and_yline_references_solve_their_operators():
    case = make_case(dims=2, n=(16, 12), fixed_axes=(1,), B=1, seed=6, stretch=0.3)
    g = case.grid()
    dt = 0.04
    C0 = R.helmholtz_operator(case, 0, g, dt)
    # no advective part: symmetric after scaling by the cell volume, and the same matrix whatever the velocity field
    D = sp.diags(g.det.ravel())
    S = (D @ C0).toarray()
    assert np.abs(S - S.T).max() < 1e-10 * np.abs(S).max()
    r = np.random.default_rng(2).standard_normal((2, C0.shape[0]))
    z = R.solve(C0, r)
    assert np.abs(C0 @ z.T - r.T).max() < 1e-10 * np.abs(r).max()
    C, _, _ = O.build_advection_matrix(case.oracle_domain(0, g), dt)
    T = R.yline_operator(C, case.shape)
    Cd = sp.csr_matrix(C).toarray()
    Td = T.toarray()
    ny, nx = case.shape
    for i in range(C.shape[0]):
        for k in range(C.shape[0]):
            same_col = (i % nx) == (k % nx)
            dj = k // nx - i // nx
            keep = same_col and abs(dj) <= 1
            assert Td[i, k] == (Cd[i, k] if keep else 0.0)
