"""Conditions on the inputs of the normal-flux parity tests (``tests/helpers.py::with_normal_flux``), checked on the oracle alone:
the boundary fluxes balance (the pressure system stays compatible), the oracle's step stays finite, the normal flux really moves
the quantities the GPU tests compare, and the advection matrix -- hence every Krylov system of the suite -- does not change."""
import numpy as np
import pytest

from oracle import piso_oracle as O
from tests.helpers import NORMAL_FLUX_CASES, NORMAL_FLUX_DT, normal_flux_case, rel_err, slab_areas


@pytest.mark.parametrize("name", list(NORMAL_FLUX_CASES))
def test_normal_flux_inputs_are_balanced_and_matter(name):
    case, plain = normal_flux_case(name), normal_flux_case(name, normal_flux=False)
    g = case.grid()
    d = case.dims
    assert np.array_equal(case.velocity, plain.velocity)
    for f in case.fixed_faces:
        a = f >> 1
        for c in range(d):
            if c != a:
                assert np.array_equal(case.bvel[f][:, c], plain.bvel[f][:, c])      # tangential components left alone
        assert np.all(plain.bvel[f][:, a] == 0.0) and np.abs(case.bvel[f][:, a]).min() > 0.0
        # zero-mean random part + the through-flow of the axis, whose direction differs between the envs
        area = slab_areas(case, f)
        for b in range(case.B):
            mean = float((case.bvel[f][b, a] * area).sum() / area.sum())
            assert abs(mean - 0.2 * (a + 1) * (-1) ** b) < 1e-14
    for b in range(case.B):
        dt = NORMAL_FLUX_DT[b]
        dom, dom0 = case.oracle_domain(b, g), plain.oracle_domain(b, g)
        assert abs(O.boundary_flux_balance(dom)) < 1e-12
        _, A, offs = O.build_advection_matrix(dom, dt)
        _, A0, offs0 = O.build_advection_matrix(dom0, dt)
        assert np.array_equal(A, A0) and all(np.array_equal(x, y) for x, y in zip(offs, offs0))
        assert rel_err(O.advection_rhs_velocity(dom, dt), O.advection_rhs_velocity(dom0, dt)) > 1e-2
        assert rel_err(O.divergence(dom, dom.velocity), O.divergence(dom0, dom0.velocity)) > 1e-2
        if case.scalar is not None:
            assert rel_err(O.advection_rhs_scalar(dom, dt), O.advection_rhs_scalar(dom0, dt)) > 1e-2
        O.piso_split_step(dom, dt)
        assert np.isfinite(dom.velocity).all() and np.isfinite(dom.pressure).all()
        assert dom.scalar is None or np.isfinite(dom.scalar).all()
