"""Per-env viscosity / diffusivity without a GPU: the ABI, what ``Domain`` keeps, the argument errors of the envs, and the per-env
Nusselt factor and wall-shear coefficient on the CPU stand-in solver (tests/stub_solver.py)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import fluidgym_amd
from fluidgym_amd import _lib as L
from fluidgym_amd.simulation import domain as domain_mod
from fluidgym_amd.simulation.domain import Domain
from tests.stub_solver import StubSolver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["fg_set_viscosity_batch", "fg_set_scalar_viscosity_batch", "fg_mb_set_viscosity_batch", "fg_mb_wall_forces_batch"]


class PerEnvStub(StubSolver):
    """The stand-in with the setters of the real solver: a float or one value per env."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.dtype = kw.get("dtype", torch.float32)
        self.viscosity_B, self.scalar_viscosities, self.scalar_viscosities_B = None, {}, {}

    def set_viscosity(self, nu):
        t = torch.as_tensor(nu, dtype=torch.float64).reshape(-1)
        self.viscosity_B = t.clone() if t.numel() > 1 else None
        self.viscosity = float(t[0])

    def set_scalar_viscosity(self, ch, k):
        t = torch.as_tensor(k, dtype=torch.float64).reshape(-1)
        self.scalar_viscosities_B[ch] = t.clone() if t.numel() > 1 else None
        self.scalar_viscosities[ch] = float(t[0])


@pytest.fixture
def stub(monkeypatch):
    monkeypatch.setattr(domain_mod, "NativeSolver", PerEnvStub)


def test_header_and_libraries_export_the_new_entries():
    header = open(os.path.join(ROOT, "include", "fluidgym_hip.h")).read()
    for lib, sigs in ((L.load(), L.SIGNATURES), (L.load_f64(), L.SIGNATURES_F64)):
        for name in NEW:
            assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
            assert name in sigs and getattr(lib, name) is not None
    assert "fg_envglue_channel_observe_batch" in L.SIGNATURES and re.search(r"\bint\s+fg_envglue_channel_observe_batch\s*\(", header)
    # by-value viscosities of the fp64 build are doubles, the arrays are pointers in both
    assert L.SIGNATURES_F64["fg_mb_wall_forces_batch"][1][7] is ctypes.c_double
    assert L.SIGNATURES["fg_set_viscosity_batch"][1][1] is ctypes.c_void_p
    # a null handle is refused, not dereferenced
    assert L.load().fg_set_viscosity_batch(None, None) < 0
    assert L.load().fg_mb_set_viscosity_batch(None, None) < 0


def test_domain_keeps_a_per_env_viscosity(stub):
    nu = torch.tensor([0.02, 0.05, 0.1])
    dom = Domain(2, nu, passiveScalarChannels=1, device="cpu", batch=3)
    assert dom.heterogeneous and dom.viscosity.shape == (3,) and torch.allclose(dom.viscosity, nu)
    one = Domain(2, torch.tensor([0.05]), device="cpu", batch=3)       # one element: what it always meant
    assert not one.heterogeneous and one.viscosity.shape == (1,) and float(one.viscosity) == pytest.approx(0.05)
    assert Domain(2, 0.05, device="cpu", batch=3).viscosity.shape == (1,)
    with pytest.raises(ValueError, match="viscosity"):
        Domain(2, torch.tensor([0.02, 0.05]), device="cpu", batch=3)
    dom.setScalarViscosity(torch.tensor([[0.3], [0.2], [0.1]]))      # per env: an explicit [B, C]
    from fluidgym_amd.simulation import grids
    blk = dom.CreateBlock(grids.vertex_grid([np.linspace(0, 1, 9), np.linspace(0, 1, 5)]))
    blk.CloseBoundary("-y")
    dom.PrepareSolve()
    assert torch.allclose(dom.solver.viscosity_B, nu.double()) and torch.allclose(dom.solver.scalar_viscosities_B[0], torch.tensor([0.3, 0.2, 0.1]).double())
    dom.setViscosity(0.07)
    assert not isinstance(dom._viscosity, torch.Tensor) and dom.solver.viscosity_B is None and dom.solver.viscosity == pytest.approx(0.07)
    dom.setViscosity(nu)
    from fluidgym_amd.simulation.domain_io import save_domain
    with pytest.raises(ValueError, match="per env"):
        save_domain(dom, "/nonexistent/never_written")


def test_length_and_positivity_errors_name_the_parameter():
    mk = fluidgym_amd.make
    with pytest.raises(ValueError, match="rayleigh_number"):
        mk("RBC2D-easy-v0", num_envs=3, rayleigh_number=[1e4, 2e4])
    with pytest.raises(ValueError, match="prandtl_number"):
        mk("RBC2D-easy-v0", num_envs=2, prandtl_number=[0.7, -1.0])
    with pytest.raises(ValueError, match="reynolds_number"):
        mk("CylinderJet2D-easy-v0", num_envs=2, reynolds_number=[100, 200, 300])
    with pytest.raises(ValueError, match="reynolds_number"):
        mk("CylinderRot2D-easy-v0", num_envs=2, reynolds_number=[100, 0.0])
    with pytest.raises(ValueError, match="reynolds_number"):
        mk("ChannelJet2D-v0", num_envs=2, reynolds_number=[100, 200, 300])


def test_out_of_scope_envs_refuse_sequences_with_a_clear_error():
    mk = fluidgym_amd.make
    with pytest.raises(ValueError, match="reynolds_number_wall"):
        mk("TCFSmall3D-both-easy-v0", num_envs=2, reynolds_number_wall=[180, 330])
    for env_id in ("CylinderJet3D-easy-v0", "Airfoil2D-easy-v0", "Airfoil3D-easy-v0"):
        with pytest.raises(ValueError, match="reynolds_number"):
            mk(env_id, num_envs=2, reynolds_number=[1e2, 2e2])
    from fluidgym_amd.envs.parallel_env import ParallelFluidEnv
    with pytest.raises(ValueError, match="ParallelFluidEnv"):
        ParallelFluidEnv("RBC2D-easy-v0", num_envs=2, rayleigh_number=[1e4, 2e4])


def test_one_element_means_the_scalar():
    for kw in (dict(num_envs=1), dict(), dict(num_envs=3)):
        env = fluidgym_amd.make("RBC2D-easy-v0", rayleigh_number=[4e5], **kw)
        assert not env.heterogeneous and isinstance(env._nu, float) and isinstance(env.id, str)
    dom = Domain(2, 0.05, passiveScalarChannels=1, device="cpu", batch=3)
    dom.setScalarViscosity(torch.tensor([0.3, 0.2, 0.1]))      # 1-D: per channel, as ever (one channel: its first entry)
    assert not dom.heterogeneous and dom._scalar_viscosity == [pytest.approx(0.3)]


def test_heterogeneous_batch_has_no_single_id():
    env = fluidgym_amd.make("RBC2D-easy-v0", num_envs=3, rayleigh_number=[8e4, 4e5, 8e5])
    assert env.heterogeneous
    for prop in ("id", "initial_domain_id"):
        with pytest.raises(ValueError, match="per parameter value"):
            getattr(env, prop)
    assert isinstance(fluidgym_amd.make("RBC2D-easy-v0", num_envs=3).id, str)


def test_rbc_nusselt_uses_each_envs_own_factor(stub):
    ra, pr = np.array([8e4, 4e5, 8e5]), np.array([0.7, 1.0, 2.0])
    env = fluidgym_amd.make("RBC2D-easy-v0", num_envs=3, rayleigh_number=list(ra), prandtl_number=list(pr), cuda_device="cpu")
    assert np.allclose(env._nu, np.sqrt(pr / ra)) and np.allclose(env._kappa, 1 / np.sqrt(ra * pr))
    env.seed(0)
    env._domain = env._get_domain()
    env._block = env._domain.getBlock(0)      # (the env's own initialisation resamples on the GPU: the cell volumes by hand)
    env._cell_size = torch.as_tensor(np.outer(env._block.widths[1], env._block.widths[0]))
    assert torch.allclose(env._domain.solver.viscosity_B, torch.as_tensor(np.sqrt(pr / ra)))
    assert torch.allclose(env._domain.solver.scalar_viscosities_B[0], torch.as_tensor(1 / np.sqrt(ra * pr)))
    g = torch.Generator().manual_seed(1)
    T = torch.rand(env._block.passiveScalar.shape, generator=g)
    u = torch.randn(env._block.velocity.shape, generator=g)
    T[1:], u[1:] = T[:1], u[:1]                   # the same field in every env: only the factor differs
    env._block.setPassiveScalar(T), env._block.setVelocity(u)
    nus = env.compute_global_nusselt()
    cs = env._cell_size
    mean = float((u[0, 1] * T[0, 0] * cs).sum() / cs.sum())
    for b in range(3):
        assert float(nus[b]) == pytest.approx(1.0 + np.sqrt(ra[b] * pr[b]) * mean, rel=1e-5)
    assert abs(float(nus[0] - nus[2])) > 1e-3 * abs(float(nus[0]))


def test_channel_shear_uses_each_envs_own_viscosity(stub):
    re_B = np.array([100.0, 200.0, 400.0])
    env = fluidgym_amd.make("ChannelJet2D-v0", num_envs=3, reynolds_number=list(re_B), resolution_x=32, resolution_y=16, cuda_device="cpu")
    env.seed(0)
    env._domain = env._get_domain()
    env._additional_initialization()
    assert torch.allclose(env._domain.solver.viscosity_B, torch.as_tensor(1.0 / re_B))
    u = torch.randn(env._block.velocity.shape, generator=torch.Generator().manual_seed(2))
    u[1:] = u[:1]
    env._block.setVelocity(u)
    _, shear = env._metrics_now()
    base = float(u[0, 0, 0, :].mean() + u[0, 0, -1, :].mean()) / (0.5 * env._hy)
    for b in range(3):
        assert float(shear[b]) == pytest.approx(base / re_B[b], rel=1e-5)
