"""Which advection-diffusion preconditioner ``Simulation`` asks of the native solver for the reference's flags
(``preconditionBiCG`` / ``BiCG_precondition_fallback``, PISOtorch_diff.py:449-476) -- host logic only, on the CPU stand-in of
tests/stub_solver.py.  The fp64 build carries ILU(0) alone (csrc/fg_ilu0.hip), so there the rungs are modes 4 / 5; the fp32 library
keeps the y-line solve (modes 1 / 2).  The GPU side of the same rungs: tests/test_gpu_f64_ilu0.py."""
import numpy as np
import pytest
import torch

from fluidgym_amd.simulation.domain import Domain
from fluidgym_amd.simulation.policy import set_solver_policy
from fluidgym_amd.simulation.simulation import Simulation
from tests.stub_solver import StubSolver


class _RecordingSolver(StubSolver):
    """The stand-in plus the two calls of the preconditioner policy; ``f64`` as NativeSolver reports it."""

    def __init__(self, widths, f64):
        super().__init__(widths, 1)
        self.f64 = f64
        self.modes = []

    def set_advection_preconditioner(self, mode=0):
        self.modes.append(int(mode))

    def set_double_fallback(self, on=True):
        self.double_fallback = bool(on)


def _domain(f64, n=(8, 6)):
    dom = Domain.__new__(Domain)
    widths = [np.full(k, 1.0 / k, np.float32) for k in n]
    dom.solver, dom.batch, dom.dims = _RecordingSolver(widths, f64), 1, len(n)
    return dom


@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("every,fallback", [(True, True), (True, False), (False, True), (False, False)])
def test_the_rungs_of_the_fp64_build_are_ilu0(f64, every, fallback):
    old = set_solver_policy(advection_fd_preconditioner="never")
    try:
        for n in ((8, 6), (8, 6, 4)):
            dom = _domain(f64, n)
            sim = Simulation(dom, 0.05, preconditionBiCG=every, BiCG_precondition_fallback=fallback)
            line = 1 if every else (2 if fallback else 0)
            expect = {1: 4, 2: 5}.get(line, line) if f64 else line
            assert sim.advection_preconditioner == expect and dom.solver.modes == [expect], (n, dom.solver.modes)
    finally:
        set_solver_policy(**old)


def test_fp64_rungs_refuse_an_axis_shorter_than_four_cells_by_name():
    for kw in (dict(preconditionBiCG=True), dict(BiCG_precondition_fallback=True)):
        dom = _domain(True, (8, 3))
        with pytest.raises(ValueError, match="four cells on every axis; axis 1 has 3"):
            Simulation(dom, 0.05, **kw)
        assert dom.solver.modes == []
    dom = _domain(True, (8, 6, 2))
    with pytest.raises(ValueError, match="axis 2 has 2"):
        Simulation(dom, 0.05)                     # (BiCG_precondition_fallback=True is the reference's default)
    dom = _domain(True, (8, 3))                   # without the rungs nothing needs the factorisation
    sim = Simulation(dom, 0.05, BiCG_precondition_fallback=False)
    assert sim.advection_preconditioner == 0 and dom.solver.modes == [0]
    dom = _domain(False, (8, 3))                  # the fp32 library's y-line solve takes any grid, as before
    assert Simulation(dom, 0.05).advection_preconditioner == 2


def test_fp64_refined_grid_policy_selects_ilu0_every_solve():
    """Policy ``advection_line_preconditioner`` (wall-refined grids precondition every solve): ILU(0) on the fp64 build as well."""
    old = set_solver_policy(advection_line_preconditioner=True, advection_fd_preconditioner="never")
    try:
        for f64, expect in ((False, 1), (True, 4)):
            dom = _domain(f64)
            w = np.array([0.05, 0.15, 0.3, 0.3, 0.15, 0.05], np.float32)
            dom.solver.widths[1] = w
            assert Simulation(dom, 0.05, BiCG_precondition_fallback=False).advection_preconditioner == expect
    finally:
        set_solver_policy(**old)
