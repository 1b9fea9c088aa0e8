"""Independent fp64 references for the preconditioner applications z = M^-1 r of the single-block solvers.

Every operator is taken from the oracle's matrices (``oracle/piso_oracle.py``) and solved with a sparse LU, never from product code:

- the pressure operator with A = 1 (the grid's fast-diagonalisation operator, ``csrc/fg_fdprecond.hip`` fg_fd_apply);
- the row-mean operator: the same matrix with ``A = 1 / mean_x(rA)`` per row and env (``k_fd_rowmean_factor``: with a row-constant
  1/A the oracle's face coefficients ``(alpha_P rA_P + alpha_N rA_N) / 2`` are the device's ``c_{j+1/2}``);
- the Helmholtz operator ``I/dt - nu Laplacian``: the oracle's advection-diffusion matrix with zero velocity;
- the y-line operator: the diagonal and the +-y off-diagonals of the oracle's advection-diffusion matrix, without the periodic wrap.

The pressure operators are singular (constant null space): ``r`` is made mean-free and the mean-free parts are compared.
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from oracle import piso_oracle as O


def pressure_operator(case, grid, A) -> sp.csr_matrix:
    """The oracle's pressure matrix for the coefficient field ``A`` (``A = 1``: the grid's constant-coefficient operator)."""
    A = np.broadcast_to(np.asarray(A, np.float64), grid.shape)
    P, _, _ = O.build_pressure_matrix(case.oracle_domain(0, grid), np.ascontiguousarray(A))
    return sp.csr_matrix(P)


def rowmean_A(rA: np.ndarray) -> np.ndarray:
    """``A`` of the row-mean operator: ``1 / mean_x(1/A)`` on every row (and z plane) of one env."""
    m = np.asarray(rA, np.float64).mean(axis=-1, keepdims=True)
    return np.ascontiguousarray(np.broadcast_to(1.0 / m, rA.shape))


def solve_pressure(P: sp.csr_matrix, r: np.ndarray) -> np.ndarray:
    """Mean-free ``M^-1 r`` for a pressure operator: ``r`` made mean-free, the solution pinned at cell 0 (the equation of that cell is
    the negative sum of the others, since the rows and columns of ``P`` sum to zero), then made mean-free."""
    rr = np.asarray(r, np.float64).ravel()
    rr = rr - rr.mean()
    x = np.zeros_like(rr)
    x[1:] = spla.splu(sp.csc_matrix(P[1:, 1:])).solve(rr[1:])
    return (x - x.mean()).reshape(np.shape(r))


def zero_velocity_domain(case, b: int, grid):
    """The env's domain with the velocity (and so every advective flux: the walls carry no normal velocity) set to zero."""
    dom = case.oracle_domain(b, grid)
    dom.velocity = np.zeros_like(dom.velocity)
    for f in case.fixed_faces:
        dom.bc[f].velocity = np.zeros_like(dom.bc[f].velocity)
    return dom


def helmholtz_operator(case, b: int, grid, dt: float) -> sp.csr_matrix:
    """``I/dt - nu Laplacian`` of the velocity system: the oracle's advection-diffusion matrix at zero velocity."""
    C, _, _ = O.build_advection_matrix(zero_velocity_domain(case, b, grid), dt)
    return sp.csr_matrix(C)


def yline_operator(C: sp.csr_matrix, shape) -> sp.csr_matrix:
    """The diagonal and the +-y neighbours of ``C`` (cells in natural order, x fastest), without the periodic wrap along y."""
    C = sp.csr_matrix(C)
    ny, nx = shape[-2], shape[-1]
    n = int(np.prod(shape))
    idx = np.arange(n)
    j = (idx // nx) % ny
    rows, cols = [idx], [idx]
    lo, hi = idx[j > 0], idx[j < ny - 1]
    rows += [lo, hi]
    cols += [lo - nx, hi + nx]
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    vals = np.asarray(C[rows, cols]).ravel()
    return sp.csr_matrix((vals, (rows, cols)), shape=(n, n))


def solve(M: sp.csr_matrix, r: np.ndarray) -> np.ndarray:
    """``M^-1 r`` for a nonsingular operator; ``r`` shaped ``[k, N]`` or ``[N]`` (k right-hand sides)."""
    lu = spla.splu(sp.csc_matrix(M))
    r = np.asarray(r, np.float64)
    if r.ndim == 1:
        return lu.solve(r)
    return np.stack([lu.solve(v) for v in r])


def rel_err(a: np.ndarray, b: np.ndarray) -> float:
    """``max |a - b| / max |b|``."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))
