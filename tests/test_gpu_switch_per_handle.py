"""The switches of csrc/fg_switches.h are read per HANDLE, at fg_create: two handles created one after the other in ONE process under
different values each run under their own (FG_JAC_SWEEPS, FG_JAC_SHAPE, FG_JAC_XCD, FG_FORCE_ZMARCH and FG_ZMARCH_SB were
function-local statics once: the first value a step met held for the process), and fg_config_dump reports every switch of the family."""
import numpy as np
import pytest
import torch

from fluidgym_amd import _lib as L
from oracle import piso_oracle as O
from tests.helpers import make_case, rel_err

pytestmark = pytest.mark.gpu


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def test_jacobi_sweeps_per_pass_belong_to_the_handle(monkeypatch):
    """The 256 x 128 case of test_gpu_jacobi.py::test_sweeps_started_from_the_block_velocity: a solve ends at a pass boundary, so
    used_iterations + 1 is a multiple of the handle's sweeps per pass (jac_mark, fg_jacobi.hip)."""
    n, B = (256, 128), 2
    h = min(2.0 / n[0], 1.0 / n[1])
    case = make_case(dims=2, n=n, fixed_axes=(0, 1), B=B, seed=6, stretch=0.0, nu=0.25 * h, vel_scale=0.5)
    dt = [0.2 * h, 0.1 * h]
    tol = 2e-7 / 0.1 / h
    for sweeps in (4, 6):
        monkeypatch.setenv("FG_JAC_SWEEPS", str(sweeps))
        ns = case.native()
        assert ns.config_dump()["FG_JAC_SWEEPS"] == sweeps
        ns.set_advection_jacobi(True)
        ns.set_advection_start(False)
        ns.setup_advection(dt)
        info = ns.solve_advection(tol=tol)
        torch.cuda.synchronize()
        x = _np(ns.buffer(3, (B, 2) + case.shape))
        assert ns.advection_jacobi_counts() == {"settled_by_sweeps": 1, "handed_to_bicgstab": 0}
        ns.close()
        print(f"FG_JAC_SWEEPS={sweeps}: sweeps used", [i.used_iterations + 1 for i in info])
        for b in range(B):
            dom = case.oracle_domain(b, case.grid())
            C, _, _ = O.build_advection_matrix(dom, dt[b])
            rhs = O.advection_rhs_velocity(dom, dt[b])
            for c in range(2):
                i = info[2 * b + c]
                assert i.used_iterations + 1 > 0 and (i.used_iterations + 1) % sweeps == 0, (sweeps, b, c, i.used_iterations)
                res = float(np.sqrt(np.mean((rhs[c].ravel() - C @ x[b, c].ravel()) ** 2)))
                assert i.converged and res < 2.5 * tol, (sweeps, b, c, res, tol)


def test_zmarch_chunk_belongs_to_the_handle(monkeypatch):
    """The smallest grid of test_gpu_parity.py::test_zmarch_3d_kernels_match_brick_kernels_and_oracle: the first handle runs the
    z-march kernels with chunks of 8 planes, the second the brick kernels.  Same operator, same right-hand side: the applications agree to
    that test's 1e-5, and each CG solution leaves a true residual below its 1e-5 under the OTHER handle's operator."""
    case = make_case(dims=3, n=(64, 32, 32), fixed_axes=(1,), B=2, seed=5, stretch=0.3)
    rng = np.random.default_rng(1)
    d = lambda a: torch.from_numpy(a).cuda()
    rA = d(rng.uniform(0.6, 1.4, size=(2,) + case.shape).astype(np.float32))
    x0 = d(rng.standard_normal((2,) + case.shape).astype(np.float32))
    b_ = rng.standard_normal((2,) + case.shape)
    b_ = d((b_ - b_.mean(axis=(1, 2, 3), keepdims=True)).astype(np.float32))
    handles, y, x = {}, {}, {}
    for force in (8, -1):
        monkeypatch.setenv("FG_FORCE_ZMARCH", str(force))
        ns = handles[force] = case.native()
        assert ns.config_dump()["FG_FORCE_ZMARCH"] == force
        y[force] = ns.poisson_apply(rA, x0).clone()
        x[force] = torch.zeros_like(x0)
        info = ns.poisson_cg(rA, b_, x[force], tol=1e-6)
        torch.cuda.synchronize()
        assert all(i.converged for i in info)
    assert handles[8].config_dump()["FG_FORCE_ZMARCH"] == 8      # (still its own, after the second handle was created)
    assert rel_err(_np(y[8]), _np(y[-1])) < 1e-5
    for force in (8, -1):
        res = _np(b_) - _np(handles[-1 if force == 8 else 8].poisson_apply(rA, x[force]))
        rms = np.sqrt((res ** 2).mean(axis=(1, 2, 3)))
        print(f"FG_FORCE_ZMARCH={force}: true residual under the other handle's operator", rms)
        assert (rms < 1e-5).all(), (force, rms)
    for ns in handles.values():
        ns.close()


def test_single_block_dump_holds_every_switch_of_its_family(monkeypatch):
    monkeypatch.setenv("FG_DEV_DT", "0")
    monkeypatch.setenv("FG_FD_FACFUSE", "0")
    case = make_case(dims=2, n=(64, 16), fixed_axes=(1,), B=2, seed=1)
    ns = case.native()
    cfg = ns.config_dump()
    want = L.read_json(ns.lib.fg_switch_values, 0, lib=ns.lib)
    ns.close()
    assert set(cfg) >= set(want)
    assert {k: cfg[k] for k in want} == want and cfg["FG_DEV_DT"] == 0 and cfg["FG_FD_FACFUSE"] == 0      # (no call has changed one since create)
    assert not set(cfg) & {"FG_CG_WGS_PER_SLOT", "FG_TRIDIAG_CB", "FG_HELM_CB"}
