"""Rayleigh-Benard convection envs (2-D / 3-D), batched.

Follows ``envs/rbc/rbc_env_base.py`` and ``envs/rbc/rbc_env_2d.py`` / ``rbc_env_3d.py`` of the
reference:

* grid: wall-refined orthogonal, ``x = resolution * n_heaters``, ``y = round(2 x / (aspect pi))``,
  ``L = H aspect pi`` with ``H = 1``, base 1.02 (``rbc_env_base.py:114-117, 176-198``); periodic in x
  (and z), FIXED plates at ``+-y`` with Dirichlet temperature ``T_hot = 1`` / ``T_cold = 0``;
* ``nu = sqrt(Pr/Ra)``, ``kappa = 1/sqrt(Ra Pr)`` (``:181-186``); temperature is passive scalar 0 and
  acts back through the Boussinesq source ``S = [0, T, (0)]`` set in the ``PRE_VELOCITY_SETUP`` hook
  (``:285-297``) -- here the fused native form (``fg_step_options.buoyancy_*``);
* solver settings ``:301-325`` (adaptive CFL, 2 correctors, pressure tol 1e-5, best-result);
* initial state: linear conduction profile + 0.1 N(0,1) clamped to [T_cold, T_hot], velocity
  0.05 N(0,1) (``:216-267``); randomisation = flip / roll / noise / 1-2 time units of simulation
  (``:335-398``);
* action -> bottom-plate temperature: zero-mean shift, ``T / max(|T|,1) * heater_limit`` limiter
  and cubic blending between heaters (``rbc_env_2d.py:196-276``);
* reward ``nu_ref - Nu`` with ``Nu = 1 + sqrt(Ra Pr) <u_y T>_V`` (``rbc_env_base.py:491-513, 579-595``).

Observations follow the reference path: fields are resampled to the render grid
(``_resample_block_data`` -> ``SampleTransformedGridLocalToGlobalMulti``, here ``fg_resample`` through
``fluidgym_amd.simulation.resample.UniformResampler``, fill 16 passes as ``rbc_env_base.py:324-325``) and read at
the integer sensor positions of ``_get_sensor_locations_2d`` / ``rbc_env_3d.py:182-199``.
"""
from __future__ import annotations

from typing import Any, Dict

import numpy as np
import torch

from .. import spaces
from ..simulation import grids
from ..simulation.domain import Domain
from ..simulation.resample import UniformResampler
from ..simulation.simulation import Simulation
from . import obs_extraction as X
from .flow_statistics import FlowStatisticsMixin
from .fluid_env import FluidEnv, is_per_env, per_env_parameter

RBC_2D_DEFAULT_CONFIG = {
    "rayleigh_number": 8e4,
    "prandtl_number": 0.7,
    "n_heaters": 12,
    "resolution": 8,
    "dt": 0.05,
    "adaptive_cfl": 0.8,
    "step_length": 1.0,
    "episode_length": 200,
    "local_obs_window": 11,
    "local_reward_weight": 0.2,
    "uniform_grid": False,
    "aspect_ratio": 1.0,
    "use_marl": False,
    "dtype": torch.float32,
    "load_initial_domain": True,      # (as the reference; without files on disk the state is generated, fluid_env.py here)
    "load_domain_statistics": True,
    "randomize_initial_state": True,
    "enable_actions": True,
    "differentiable": False,
}

RBC_3D_DEFAULT_CONFIG = {          # rbc_env_3d.py's default config (held by tests/golden/reference_registry.json)
    **RBC_2D_DEFAULT_CONFIG,
    "rayleigh_number": 6e3,
    "n_heaters": 8,
    "resolution": 8,
    "adaptive_cfl": 0.5,
    "dt": 0.05,
    "local_obs_window": 3,
    "local_reward_weight": 0.0015,
    "use_marl": True,
}


def _nusselt_factor(rayleigh_number, prandtl_number, like: torch.Tensor):
    """``sqrt(Ra Pr)``: a float, or -- with one Ra / Pr per env -- env b's own value shaped to broadcast against ``like [B, ...]``."""
    f = np.sqrt(rayleigh_number * prandtl_number)
    if np.ndim(f) == 0:
        return float(f)
    t = torch.as_tensor(np.ascontiguousarray(f), dtype=like.dtype, device=like.device)
    return t.reshape((t.numel(),) + (1,) * (like.dim() - 1))


class RBCEnvBase(FlowStatisticsMixin, FluidEnv):
    _supports_marl = True
    _flow_stats_scalar = True           # start_flow_statistics records the temperature as channel T
    _resolution_scale_y: float = 2.0
    _non_uniform_grid_base = 1.02
    _H: float = 1.0
    _T_hot: float = 1.0
    _T_cold: float = 0.0
    _heater_limit: float = 0.75
    _buoyancy_factor: float = 1.0
    _n_sensors_per_heater: int = 4
    _n_sensors_y: int = 8
    _metrics = ["nusselt"]
    _initial_domain_restart = True      # rbc_env_base.py:126: one development per mode

    def __init__(self, rayleigh_number, prandtl_number, n_heaters, resolution, dt, adaptive_cfl, step_length,
                 episode_length, ndims, local_obs_window=11, local_reward_weight=None, uniform_grid=False,
                 aspect_ratio=1.0, **kw):
        # a number (as ever) or one value per env of the batch: Ra / Pr then become float64 arrays [num_envs] and everything
        # derived from them below is per env
        rayleigh_number = per_env_parameter("rayleigh_number", rayleigh_number, kw.get("num_envs"))
        prandtl_number = per_env_parameter("prandtl_number", prandtl_number, kw.get("num_envs"))
        self._heterogeneous = is_per_env(rayleigh_number) or is_per_env(prandtl_number)
        self._rayleigh_number = rayleigh_number
        self._prandtl_number = prandtl_number
        self._local_obs_window = int(local_obs_window)
        self._local_reward_weight = local_reward_weight
        self._heater_width = int(resolution)
        self._n_heaters = int(n_heaters)
        self._uniform_grid = uniform_grid
        self._aspect_ratio = aspect_ratio * np.pi
        self._x = int(resolution * n_heaters)
        self._y = round(self._resolution_scale_y * self._x / self._aspect_ratio)
        self._L = self._H * self._aspect_ratio
        if self._heterogeneous:
            n_envs = int(kw.get("num_envs") or 1)
            self._nu = np.broadcast_to((prandtl_number / rayleigh_number) ** 0.5, (n_envs,)).copy()
            self._kappa = np.broadcast_to((rayleigh_number * prandtl_number) ** -0.5, (n_envs,)).copy()
        else:
            self._nu = float((prandtl_number / rayleigh_number) ** 0.5)
            self._kappa = float((rayleigh_number * prandtl_number) ** -0.5)
        super().__init__(dt=dt, adaptive_cfl=adaptive_cfl, step_length=step_length, episode_length=episode_length,
                         ndims=ndims, **kw)

    # ---- spaces ---------------------------------------------------------------------------
    @property
    def _n_sensors_x(self) -> int:
        return self._n_heaters * self._n_sensors_per_heater

    @property
    def n_agents(self) -> int:
        """rbc_env_base.py:418-428."""
        if not self._use_marl:
            return 1
        return self._n_heaters if self._ndims == 2 else self._n_heaters ** 2

    def _get_action_space(self):
        """Per-agent action space (rbc_env_2d.py:112-129, rbc_env_3d.py:120-134)."""
        if self._use_marl:
            shape = (1,)
        else:
            shape = (self._n_heaters, 1) if self._ndims == 2 else (self._n_heaters, self._n_heaters, 1)
        return spaces.Box(low=-1.0, high=1.0, shape=shape, dtype=np.float32)

    def _get_observation_space(self):
        """Per-agent observation space (rbc_env_2d.py:131-166, rbc_env_3d.py:136-172)."""
        nx = self._n_sensors_per_heater * (self._local_obs_window if self._use_marl else self._n_heaters)
        shape = (self._n_sensors_y, nx) if self._ndims == 2 else (nx, self._n_sensors_y, nx)
        return spaces.Dict({
            "temperature": spaces.Box(low=self._T_cold, high=self._T_hot + self._heater_limit, shape=shape, dtype=np.float32),
            "velocity": spaces.Box(low=-np.inf, high=np.inf, shape=(self._ndims,) + shape, dtype=np.float32),
            "pressure": spaces.Box(low=-np.inf, high=np.inf, shape=shape, dtype=np.float32),
        })

    # ---- domain ---------------------------------------------------------------------------
    def _edges(self):
        base = 1.0 if self._uniform_grid else self._non_uniform_grid_base
        e = grids.wall_refined_edges(self._x, self._y, (0, -self._H / 2), (self._L, self._H / 2), ["-y", "+y"], base)
        if self._ndims == 3:
            e.append(grids.lerp_edges(0.0, self._L, grids.weights_linear(self._x)))
        return e

    def _get_domain(self) -> Domain:
        coords = grids.vertex_grid(self._edges())
        as_t = lambda v: torch.as_tensor(v, dtype=torch.float64) if self._heterogeneous else torch.tensor([v])
        dom = Domain(self._ndims, as_t(self._nu), passiveScalarChannels=1, name="RBCDomain",
                     device=self._cuda_device, dtype=self._dtype, batch=self._num_envs)
        dom.setScalarViscosity(as_t(self._kappa).reshape(-1, 1) if self._heterogeneous else as_t(self._kappa))
        blk = dom.CreateBlock(vertexCoordinates=coords, name="RBCBlock")
        blk.CloseBoundary("-y")
        blk.CloseBoundary("+y")
        dom.PrepareSolve()
        blk.getBoundary("-y").setPassiveScalar(torch.tensor([[self._T_hot]]))
        blk.getBoundary("+y").setPassiveScalar(torch.tensor([[self._T_cold]]))
        blk.setVelocitySource(torch.zeros(1, self._ndims, *dom.solver.spatial))
        return dom

    def _get_simulation(self, domain: Domain, prep_fn: Dict[str, Any]) -> Simulation:
        return Simulation(
            domain=domain, prep_fn=prep_fn, substeps="ADAPTIVE", adaptive_CFL=self._adaptive_cfl, dt=self._dt,
            corrector_steps=2, pressure_tol=1e-5, advect_non_ortho_steps=1, pressure_non_ortho_steps=1,
            pressure_return_best_result=True, velocity_corrector="FD", non_orthogonal=False,
            buoyancy=(1, self._buoyancy_factor),  # native PRE_VELOCITY_SETUP hook (rbc_env_base.py:285-297)
        )

    def _additional_initialization(self) -> None:
        self._block = self._domain.getBlock(0)
        self._bottom_plate = self._block.getBoundary("-y")
        self._top_plate = self._block.getBoundary("+y")
        dev = self._cuda_device
        self._cell_size = self._block.getCellSizes()[0, 0]  # [(Z,)Y,X]
        # observation path: render-grid resampling + integer sensor positions (rbc_env_base.py:324-325, 445-470)
        self._resampler = UniformResampler(self._block.edges, self.render_shape[: self._ndims], fill_max_steps=16,
                                           device=dev)
        self._sensor_locations = self._get_sensor_locations().to(dev)
        seg = torch.arange(self._x, device=dev)
        self._seg_id = seg // self._heater_width
        self._x_pos = seg % self._heater_width

    def _fill_initial_fields(self) -> None:
        dev, B = self._cuda_device, self._num_envs
        grad = torch.linspace(self._T_hot, self._T_cold, steps=self._y, device=dev)
        shape = [1] * (self._ndims + 2)
        shape[-2] = self._y
        T = grad.view(shape).expand(B, 1, *self._domain.solver.spatial).clone()
        T += torch.randn(T.shape, device=dev, generator=self._torch_rng_cuda) * 0.1 * (self._T_hot - self._T_cold)
        T.clamp_(self._T_cold, self._T_hot)
        self._block.setPassiveScalar(T)
        u = torch.randn(self._block.velocity.shape, device=dev, generator=self._torch_rng_cuda) * 0.05
        self._block.setVelocity(u)
        self._block.pressure.zero_()
        self._domain.solver.reset_solver_state()

    def _randomize_domain(self) -> None:
        """rbc_env_base.py:335-398 (flip, roll, noise, 1..2 time units of simulation), per batch."""
        T, u = self._block.passiveScalar, self._block.velocity
        if self._np_rng.uniform(0.0, 1.0) > 0.5:
            T.copy_(torch.flip(T, dims=[-1]))
            u.copy_(torch.flip(u, dims=[-1]))
            u[:, 0] *= -1.0
        if self._ndims == 3 and self._np_rng.uniform(0.0, 1.0) > 0.5:      # 3-D: the z axis too (rbc_env_base.py:350-353)
            T.copy_(torch.flip(T, dims=[-3]))
            u.copy_(torch.flip(u, dims=[-3]))
            u[:, 2] *= -1.0
        shift = int(self._np_rng.integers(0, self._x))
        T.copy_(torch.roll(T, shifts=shift, dims=-1))
        u.copy_(torch.roll(u, shifts=shift, dims=-1))
        if self._ndims == 3:                                                # (:359-362)
            z_shift = int(self._np_rng.integers(0, self._x))
            T.copy_(torch.roll(T, shifts=z_shift, dims=-3))
            u.copy_(torch.roll(u, shifts=z_shift, dims=-3))
        T.add_(torch.randn(T.shape, device=T.device, generator=self._torch_rng_cuda) * 0.05).clamp_(self._T_cold, self._T_hot)
        u.add_(torch.randn(u.shape, device=u.device, generator=self._torch_rng_cuda) * 0.05)
        sim_time = self._np_rng.uniform(1.0, 2.0)
        for _ in range(int(sim_time / self._dt)):
            self._sim.single_step()

    def _reset_symmetries(self):
        """rbc_env_base.py:335-362: mirror and roll along x, and along z in 3-D -- the axes the block holds as periodic."""
        rolls = self._periodic_rolls()
        return tuple(k for k in ("flip_x", "flip_z", "shift_x", "shift_z") if "shift_" + k[-1] in rolls)

    def _reset_envs_noise(self, envs: torch.Tensor) -> None:
        """The noise of ``_randomize_domain`` (0.05 on T, clamped, and on u) for the envs ``envs`` only."""
        T, u = self._block.passiveScalar, self._block.velocity
        n = (int(envs.numel()),)
        T.index_add_(0, envs, torch.randn(n + tuple(T.shape[1:]), device=T.device, generator=self._torch_rng_cuda).to(T.dtype) * 0.05)
        T.index_copy_(0, envs, T.index_select(0, envs).clamp_(self._T_cold, self._T_hot))
        u.index_add_(0, envs, torch.randn(n + tuple(u.shape[1:]), device=u.device, generator=self._torch_rng_cuda).to(u.dtype) * 0.05)

    # ---- control --------------------------------------------------------------------------
    def _smooth_profile(self, T_action: torch.Tensor) -> torch.Tensor:
        """Cubic blending between neighbouring heaters over 10 % of the heater width along the LAST axis
        (rbc_env_2d.py:196-237, rbc_env_3d.py:201-239); ``T_action [..., n_heaters] -> [..., x]``."""
        hw = self._heater_width
        bw = round(hw * 0.1)
        T1 = T_action[..., self._seg_id]
        if bw == 0:
            return T1
        T0 = torch.roll(T_action, 1, dims=-1)[..., self._seg_id]
        T2 = torch.roll(T_action, -1, dims=-1)[..., self._seg_id]
        tL = (self._x_pos.float() / bw + 0.5).clamp(0.0, 1.0)
        tR = 1 - torch.roll(tL, shifts=hw - bw + 1, dims=0)
        blend = lambda t, A, Bv: (1 - t * t * (3 - 2 * t)) * A + (t * t * (3 - 2 * t)) * Bv
        left = self._x_pos < bw
        right = self._x_pos >= hw - bw
        return torch.where(left, blend(tL, T0, T1), torch.where(right, blend(tR, T1, T2), T1))

    def _action_to_control(self, action: torch.Tensor) -> torch.Tensor:
        a = action.reshape(self._num_envs, -1)
        shifted = a - a.mean(dim=1, keepdim=True)  # eq. (8) of Vignon et al. 2023
        T = shifted / (torch.clamp(shifted.abs(), min=1.0) / self._heater_limit) + self._T_hot  # eq. (9)
        return T

    def _apply_action(self, action: torch.Tensor) -> None:
        T = self._action_to_control(action)
        if self._ndims == 2:
            control = self._smooth_profile(T).view(self._num_envs, 1, 1, self._x)
        else:
            # [z-heater, x-heater] (rbc_env_3d.py:246-268): smooth along z, then along x
            Th = T.view(self._num_envs, self._n_heaters, self._n_heaters)
            sz = self._smooth_profile(Th.transpose(1, 2)).transpose(1, 2)     # [B, Z, x-heater]
            control = self._smooth_profile(sz).view(self._num_envs, 1, self._x, 1, self._x)
        self._bottom_plate.setPassiveScalar(control)

    def plot_actuation(self, *args, **kwargs) -> None:
        raise NotImplementedError("plot_actuation: plotting is not part of fluidgym_amd")

    # ---- observation / reward -------------------------------------------------------------
    @property
    def render_shape(self):
        """(nx, height, nx) of the rendered / resampled domain (rbc_env_base.py:399-405)."""
        nx = self._n_heaters * 20
        return (nx, round(nx / self._aspect_ratio), nx)

    def _get_sensor_locations(self) -> torch.Tensor:
        """Integer render-grid positions of the sensors, ``[ndims, n]`` with x fastest-varying last
        (rbc_env_base.py:445-470; rbc_env_3d.py:182-199)."""
        nx, ny = self.render_shape[:2]
        sx = torch.linspace(0, nx, self._n_sensors_x + 1)[:-1] + nx / (2 * self._n_sensors_x)
        sy = torch.linspace(0, ny, self._n_sensors_y + 1)[:-1] + ny / (2 * self._n_sensors_y)
        gx, gy = torch.meshgrid(sx, sy, indexing="ij")
        loc = torch.stack([gx, gy], dim=-1).reshape(-1, 2).T.round().to(torch.int64)
        if self._ndims == 2:
            return loc
        nz = self.render_shape[-1]
        nsz = self._n_sensors_per_heater * self._n_heaters
        sz = (torch.linspace(0, nz, nsz + 1)[:-1] + nz / (2 * nsz)).round().to(torch.int64)
        return torch.stack([loc[0].repeat_interleave(nsz), loc[1].repeat_interleave(nsz), sz.repeat(loc.shape[1])], dim=0)

    def get_temperature(self) -> torch.Tensor:
        """Temperature on the render grid ``[B, (oz,) oy, ox]`` (rbc_env_base.py:472-489, batched)."""
        return self._resampler(self._block.passiveScalar)[:, 0]

    def get_velocity(self) -> torch.Tensor:
        """Velocity on the render grid ``[B, d, (oz,) oy, ox]`` (fluid_env.py:658-681, batched)."""
        return self._resampler(self._block.velocity)

    def get_pressure(self) -> torch.Tensor:
        """Pressure on the render grid ``[B, (oz,) oy, ox]`` (fluid_env.py:683-706, batched)."""
        return self._resampler(self._block.pressure)[:, 0]

    def _diagnostic_to_view(self, cells: torch.Tensor) -> torch.Tensor:
        return self._resampler(cells)

    def _frame_specs(self):
        """rbc_env_base.py:541-577: the temperature between ``T_cold`` and ``T_hot + heater_limit`` in ``rainbow``; the planes and
        their orientation are ``frames.rbc_frame_specs``."""
        from .frames import rbc_frame_specs

        T = self.get_temperature().unsqueeze(1)
        rng = (self._T_cold, self._T_hot + self._heater_limit)
        return {key: (T, spec, rng, "rainbow", None) for key, spec in rbc_frame_specs(self._ndims, T.shape[2:]).items()}

    def _frame_specs_3d(self):
        """rbc_env_3d.py:511-527: the temperature as a volume between ``T_cold`` and ``T_hot + heater_limit``, ``rainbow``, the
        opacity of a sample the reference's ``log1p`` of the normalised value (``render3d.log_opacity_table``), elev 15, azim 45; the
        box has the proportions of the render grid, as ``set_box_aspect(field.shape)`` gives it there."""
        from .render3d import log_opacity_table

        T = self.get_temperature().unsqueeze(1)
        return {"3d_temperature": dict(mode="volume", view=T, channel=0, range=(self._T_cold, self._T_hot + self._heater_limit),
                                       cmap="rainbow", opacity=log_opacity_table(), extent=tuple(float(v) for v in self.render_shape),
                                       elev=15, azim=45)}

    def _get_global_obs(self):
        """rbc_env_2d.py:175-194 / rbc_env_3d.py:291-330 with a leading env axis."""
        B, d = self._num_envs, self._ndims
        sl = self._sensor_locations
        T, u, p = self.get_temperature(), self.get_velocity(), self.get_pressure()
        nsx, nsy = self._n_sensors_x, self._n_sensors_y
        if d == 2:
            pick = lambda t: t[..., sl[1], sl[0]]
            return {
                "temperature": pick(T).reshape(B, nsx, nsy).transpose(1, 2),
                "velocity": pick(u).reshape(B, 2, nsx, nsy).transpose(2, 3),
                "pressure": pick(p).reshape(B, nsx, nsy).transpose(1, 2),
            }
        pick = lambda t: t[..., sl[2], sl[1], sl[0]]
        return {
            "temperature": pick(T).reshape(B, nsx, nsy, nsx).permute(0, 3, 2, 1),
            "velocity": pick(u).reshape(B, 3, nsx, nsy, nsx).permute(0, 1, 4, 3, 2),
            "pressure": pick(p).reshape(B, nsx, nsy, nsx).permute(0, 3, 2, 1),
        }

    def compute_global_nusselt(self) -> torch.Tensor:
        """``Nu = 1 + sqrt(Ra Pr) * <u_y T>_V`` (rbc_env_base.py:491-536), per env ``[B]``."""
        T = self._block.passiveScalar[:, 0]
        uy = self._block.velocity[:, 1]
        dims = tuple(range(1, self._ndims + 1))
        mean = (uy * T * self._cell_size).sum(dim=dims) / self._cell_size.sum()
        return 1.0 + _nusselt_factor(self._rayleigh_number, self._prandtl_number, mean) * mean

    @property
    def nu_ref(self) -> float:
        """rbc_env_base.py:408-416: the median of the uncontrolled Nusselt number in 2-D, its mean in 3-D; 0 without statistics."""
        s = self._metric_stat("nusselt")
        if s is None:
            return 0.0
        return float(s.p50 if self._ndims == 2 else s.mean)

    def _local_nusselt(self, T, u_y, cell_size):
        """``_compute_nusselt`` on per-agent windows (rbc_env_base.py:491-513): ``T, u_y [B, n_agents, *win]``."""
        dims = tuple(range(2, T.dim()))
        mean = (u_y * T * cell_size).sum(dim=dims) / cell_size.sum()
        return 1.0 + _nusselt_factor(self._rayleigh_number, self._prandtl_number, mean) * mean

    def _get_local_obs(self):
        """rbc_env_2d.py:280-325 / rbc_env_3d.py:330-385 with a leading env axis: ``[B, n_agents, ...]``."""
        g = self._get_global_obs()
        nh, w, W = (self._n_heaters, self._n_sensors_per_heater, self._local_obs_window)
        win = (lambda f: X.extract_moving_window_2d(f, nh, w, W)) if self._ndims == 2 else \
              (lambda f: X.extract_moving_window_3d(f, nh, w, W))
        u = torch.stack([win(g["velocity"][:, c]) for c in range(self._ndims)], dim=2)
        return {"temperature": win(g["temperature"]), "velocity": u, "pressure": win(g["pressure"])}

    def _get_local_rewards(self) -> torch.Tensor:
        """Local Nusselt numbers over each agent's window of the simulation grid (rbc_env_2d.py:327-358,
        rbc_env_3d.py:387-424), ``[B, n_agents]``."""
        nh, hw, W = self._n_heaters, self._heater_width, self._local_obs_window
        T, uy, cs = self._block.passiveScalar[:, 0], self._block.velocity[:, 1], self._cell_size
        if self._ndims == 2:
            lc = cs[:, : W * hw]
            lT, lu = X.extract_moving_window_2d(T, nh, hw, W), X.extract_moving_window_2d(uy, nh, hw, W)
        else:
            lc = cs[: W * hw, :, : W * hw]
            lT, lu = X.extract_moving_window_3d(T, nh, hw, W), X.extract_moving_window_3d(uy, nh, hw, W)
        return self.nu_ref - self._local_nusselt(lT, lu, lc)

    def _step_marl_impl(self, action: torch.Tensor):
        """rbc_env_base.py:613-636."""
        if self._local_reward_weight is None:
            raise ValueError("local_reward_weight must be set for multi-agent step.")
        _, global_reward, terminated, info = self._step_impl(action)
        local_obs = self._get_local_obs()
        if self._local_reward_weight > 0:
            local_rewards = self._get_local_rewards()
        else:
            local_rewards = torch.zeros((self._num_envs, self.n_agents), dtype=self._dtype, device=self._cuda_device)
        w = self._local_reward_weight
        agent_rewards = w * local_rewards + (1 - w) * global_reward.unsqueeze(1)
        info["global_reward"] = global_reward
        return local_obs, agent_rewards, terminated, info

    def _step_impl(self, action: torch.Tensor):
        if self._enable_actions:
            self._apply_action(action)
        for _ in range(self._n_sim_steps):
            if not self._sim.single_step():
                raise RuntimeError("simulation step failed")
            self._after_sim_step()
        nu = self.compute_global_nusselt()
        obs = self._get_global_obs()
        return obs, self.nu_ref - nu, False, {"nusselt": nu}

    @property
    def id(self) -> str:
        self._refuse_heterogeneous_id()
        return (f"RBC{self._ndims}d_Ra{self._rayleigh_number}_Pr{self._prandtl_number}"
                f"_NH{self._n_heaters}_HW{self._heater_width}")

    @property
    def initial_domain_id(self) -> str:
        """rbc_env_base.py:605-611."""
        self._refuse_heterogeneous_id()
        return (f"rbc_{self._ndims}d_Ra{self._rayleigh_number}_Pr{self._prandtl_number}"
                f"_NH{self._n_heaters}_HW{self._heater_width}")


class RBCEnv2D(RBCEnvBase):
    _initial_domain_steps = 283      # rbc_env_2d.py:110 (uncontrolled env steps init() develops a state for)

    def __init__(self, **kw):
        super().__init__(ndims=2, **kw)


class RBCEnv3D(RBCEnvBase):
    _initial_domain_steps = 1500     # rbc_env_3d.py:118

    def __init__(self, **kw):
        super().__init__(ndims=3, **kw)
