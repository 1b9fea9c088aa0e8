"""What the cylinder and the airfoil envs share: a body in a stream on a multi-block mesh (``MeshBodyEnvBase``) and the spanwise
multi-agent layer of their 3-D variants (``SpanwiseAgentsMixin``).

The base owns the solver options both families take, the wall ring / resampler / sensor gather, the developed initial state and its
randomisation, the env-step loop (action smoothing, wall forces, their mean over the sim steps), the on-disk initial domains, the
extra state and the resampled views.  A family says what is its own through hooks: ``_get_sensor_locations``,
``_wall_ring_segments``, ``_use_pressure_multilevel``, ``_mesh_reset_warmup_env_steps``, ``_force_norm``, ``_layer_height``,
``_reward`` and ``_apply_action`` (``FluidEnv``'s), and the class attributes ``_U_mean``, ``_fill_max_steps``, ``_domain_file_name``,
``_mesh_reset_sigma`` and ``_n_controls``.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from ..simulation.resample_mb import MultiBlockResampler, MultiBlockResampler3D
from .. import spaces
from .flow_statistics import FieldStatisticsMixin, FlowStatisticsMixin
from .fluid_env import FluidEnv
from .forces import WallRing
from .inflow import InflowDisturbanceMixin
from .mesh_reset import MeshResetMixin
from .surface import SurfaceMixin
from .tracers import MeshTracerMixin


def smoothed_controls(last: torch.Tensor, target: torch.Tensor, alpha: float, n: int) -> torch.Tensor:
    """The smoothed control of ``n`` successive sim steps, ``[n, B, n_controls]`` (cylinder_env_base.py:560-566:
    ``c <- c + alpha (target - c)``): the recurrence in the operations of the per-step tensor expression (separately rounded
    multiply and add, the same type promotion)."""
    c, controls = last, []
    for _ in range(n):
        c = c + alpha * (target - c)
        controls.append(c)
    return torch.stack(controls)


class MeshBodyEnvBase(InflowDisturbanceMixin, SurfaceMixin, MeshResetMixin, MeshTracerMixin, FieldStatisticsMixin, FlowStatisticsMixin, FluidEnv):      # (multi-block: the plane statistics refuse with
                                                                                 # NotImplementedError, the per-cell ones record)
    _supports_marl = False
    _action_smoothing_alpha: float = 0.1
    _metrics = ["drag", "lift"]
    _initial_domain_steps = 400
    _n_controls = 1
    _fill_max_steps: int                # of the resampler's hole filling
    _domain_file_name: str              # the domain's name in the on-disk initial domains
    _solid_mask = None                  # device mask [ny, nx] of the pixels inside the body that the views zero, or None
    _developed = None

    def __init__(self, ndims: int, pressure_use_BiCG, pressure_deflation: bool = False, non_ortho_mode: str = "matrix",
                 initial_domain_steps: Optional[int] = None, **kw):
        if ndims not in (2, 3):
            raise ValueError("ndims must be 2 or 3")
        self._ndims = ndims
        self._pressure_use_bicg = pressure_use_BiCG
        self._pressure_deflation = bool(pressure_deflation)
        if non_ortho_mode not in ("matrix", "rhs"):
            raise ValueError("non_ortho_mode: 'matrix' (the reference's nonOrthoFlags) or 'rhs' (every cross-metric term lagged)")
        self._non_ortho_flags = 25 if non_ortho_mode == "matrix" else 10
        if initial_domain_steps is not None:
            self._initial_domain_steps = int(initial_domain_steps)
        self._sensor_locations = self._get_sensor_locations()      # (the observation space of the airfoil counts them)
        super().__init__(ndims=ndims, **kw)
        self._last_control = None

    # ---- what a family says about itself
    def _get_sensor_locations(self) -> np.ndarray:
        """Pixel (x, y) of every sensor on the render grid, ``[2, n]``; 3-D: (x, y, z), ``[3, n_sensors_z, n]``."""
        raise NotImplementedError

    def _wall_ring_segments(self) -> list:
        """``[(block, face, reversed)]`` of the body's wall, in ring order (``forces.WallRing``)."""
        raise NotImplementedError

    def _use_pressure_multilevel(self) -> bool:
        """Whether this env installs the multilevel pressure preconditioner (solver policy, per family)."""
        raise NotImplementedError

    @property
    def _force_norm(self) -> float:
        """``0.5 U^2 L``: what turns the wall force into drag and lift coefficients."""
        raise NotImplementedError

    @property
    def _layer_height(self) -> float:
        """Spanwise height of one layer of wall faces (3-D)."""
        raise NotImplementedError

    def _reward(self, cd: torch.Tensor, cl: torch.Tensor) -> torch.Tensor:
        raise NotImplementedError

    # ---- spaces: the 2-D observation
    def _get_observation_space(self):
        n = self._sensor_locations.shape[-1]
        return spaces.Dict({
            "velocity": spaces.Box(low=-np.inf, high=np.inf, shape=(n, self._ndims), dtype=np.float32),
            "pressure": spaces.Box(low=-np.inf, high=np.inf, shape=(n,), dtype=np.float32),
        })

    # ---- domain
    def _set_pressure_multilevel(self, dom) -> None:
        """``_multilevel``: the aggregate counts of the installed preconditioner, or None.  A float64 env keeps the plain recurrence
        unless policy pressure_multilevel_fp64 asks for the kernel form (policy.py)."""
        from ..simulation.policy import get_solver_policy

        self._multilevel = None
        if self._use_pressure_multilevel():
            fp64 = self._dtype == torch.float64 and get_solver_policy()["pressure_multilevel_fp64"]
            self._multilevel = dom.set_pressure_multilevel(fp64=True) if fp64 else dom.set_pressure_multilevel()

    def _additional_initialization(self) -> None:
        dom = self._domain
        self._ring = WallRing(dom, self._wall_ring_segments())
        if self._ndims == 3:
            self._resampler = MultiBlockResampler3D(self._mesh.coords, self.render_shape, fill_max_steps=self._fill_max_steps, device=dom.device)
        else:
            self._resampler = MultiBlockResampler(self._mesh.coords, self.render_shape[:2], fill_max_steps=self._fill_max_steps, device=dom.device)
        self._sensors = self._resampler.sensor_gather(self._sensor_locations.reshape(self._ndims, -1).T)
        self._deflation_cos = dom.set_pressure_deflation() if self._pressure_deflation else 1.0
        self._set_pressure_multilevel(dom)
        # the viscosity the wall-force launch takes: a float, or env b's own value [B] on the device
        self._nu_forces = (torch.as_tensor(self._nu, dtype=self._dtype, device=dom.device).contiguous() if self._heterogeneous
                           else self._nu)
        self._initial_boundary = dom.boundary_velocity.clone()  # inflow / outflow profile, walls at rest
        self._last_control = torch.zeros(self._num_envs, self._n_controls, device=dom.device, dtype=self._dtype)

    # ---- initial state
    def _develop(self) -> None:
        """Uniform stream projected onto the mesh, then ``initial_domain_steps`` uncontrolled steps (the reference ships
        states generated with 400 steps, cylinder_env_base.py:138; they are cached per env instance here)."""
        dom = self._domain
        dom.boundary_velocity.copy_(self._initial_boundary)
        dom.velocity.zero_()
        dom.velocity[:, 0] = self._U_mean
        dom.pressure.zero_()
        self._sim.make_divergence_free()
        for _ in range(self._initial_domain_steps):
            self._sim.single_step()

    def _fill_initial_fields(self) -> None:
        dom = self._domain
        if self._developed is None:
            self._develop()
            self._developed = dom.Clone()
        dom.Restore(self._developed)
        self._last_control = torch.zeros(self._num_envs, self._n_controls, device=dom.device, dtype=self._dtype)

    def _randomize_n_steps(self) -> int:
        max_n = self._mesh_reset_warmup_env_steps()
        return int(self._np_rng.integers(int(0.5 * max_n), max_n)) + 1

    def _randomize_domain(self) -> None:
        """cylinder_env_base.py:364-404, airfoil_env_base.py:327-332: noise of the family's amplitude, then a drawn number of steps."""
        n_steps = self._randomize_n_steps()
        dom, g, sigma = self._domain, self._torch_rng_cuda, self._mesh_reset_sigma
        dom.velocity.add_(torch.randn(dom.velocity.shape, device=dom.device, generator=g) * sigma)
        dom.pressure.add_(torch.randn(dom.pressure.shape, device=dom.device, generator=g) * sigma)
        for _ in range(n_steps):
            self._sim.single_step()

    # ---- observations and views
    def _get_global_obs(self) -> Dict[str, torch.Tensor]:
        dom = self._domain
        u = self._sensors(dom.velocity).to(self._dtype)   # [B, 2, S]
        p = self._sensors(dom.pressure).to(self._dtype)      # [B, S]
        return {"velocity": u.permute(0, 2, 1).contiguous(), "pressure": p}

    def _diagnostic_to_view(self, cells: torch.Tensor) -> torch.Tensor:
        v = self._resampler(cells)
        if self._solid_mask is not None:
            v[..., self._solid_mask] = 0.0
        return v

    def get_velocity(self) -> torch.Tensor:
        """Resampled velocity [B, d, (z,) y, x] (``FluidEnv.get_velocity``)."""
        return self._diagnostic_to_view(self._domain.velocity)

    def get_pressure(self) -> torch.Tensor:
        return self._resampler(self._domain.pressure)

    def render(self, *a, **kw) -> np.ndarray:
        speed = torch.linalg.vector_norm(self.get_velocity()[0], dim=0)
        if self._ndims == 3:
            speed = speed[speed.shape[0] // 2]      # mid-span slice
        return speed.detach().cpu().numpy()

    def _vortex_frame_specs(self, value_range, flip_y: bool, masks) -> Dict[str, tuple]:
        """The vorticity pictures the cylinder and airfoil envs share (cylinder_env_base.py:700-739, airfoil_env_base.py:664-702): the
        planes, with the reference's literal indices, are ``frames.vortex_frame_specs``; ``masks`` in the order of its keys."""
        from .frames import vortex_frame_specs

        w = self.get_vorticity()
        specs = vortex_frame_specs(self._ndims, w.shape[2:], flip_y)
        return {key: (w, spec, value_range, "icefire", mask) for (key, spec), mask in zip(specs.items(), masks)}

    def _vortex_frame_specs_3d(self, levels: dict, clip_x: int, solid, extent) -> Dict[str, dict]:
        """The 3-D picture the cylinder and airfoil envs share (jet_cylinder_env_3d.py:511-546, airfoil_env_3d.py:489-520): the
        surface of the vorticity magnitude at the level of the Reynolds number, coloured by the speed, ``rainbow``, the body as a
        solid, elev 10, azim 60.  The reference zeroes the vorticity in front of ``clip_x`` and in the 15 outermost rows of y: the
        clip box here."""
        re = int(self._reynolds_number)
        if re not in levels:
            raise ValueError(f"no vorticity level for Reynolds number {re}: the table has {sorted(levels)}")
        w, u = self.get_vorticity(), self.get_velocity()
        nz, ny, nx = (int(v) for v in w.shape[2:])
        return {"3d_vorticity": dict(mode="iso", view=w, channel=-1, level=levels[re], color_view=u, color_channel=-1,
                                     color_range=self._speed_range_3d(u), cmap="rainbow",
                                     clip=((clip_x, 15, 0), (nx - 1, ny - 16, nz - 1)), solid=solid, extent=extent, elev=10, azim=60)}

    # ---- forces and the env step (cylinder_env_base.py:541-776, airfoil_env_base.py:334-461, 744-776)
    def _wall_force_args(self):
        return self._nu_forces, self._layer_height

    def _get_drag_and_lift(self):
        """[B] in 2-D; [B, NZ] per spanwise layer in 3-D (face area = edge length x layer height)."""
        f = self._ring.forces(self._domain, self._nu_forces, layer_height=self._layer_height)
        return f[:, 0] / self._force_norm, f[:, 1] / self._force_norm

    def _step_impl(self, action: torch.Tensor):
        target = action.reshape(self._num_envs, self._n_controls)
        n, dev = self._n_sim_steps, self._last_control.device
        # The smoothed control of every sim step is a recurrence on a [B, n_controls] tensor: evaluated once on the host and
        # uploaded in one copy, instead of three tiny launches per sim step.  The host keeps its own copy of the last control (valid
        # while `_last_control` is the tensor this method left there), so the only read-back of a step is the action itself -- none
        # when the caller hands over a host tensor.
        mirror = getattr(self, "_last_control_mirror", None)
        c = mirror[1] if mirror is not None and mirror[0] is self._last_control else self._last_control.cpu()
        host = smoothed_controls(c, target.cpu(), self._action_smoothing_alpha, n)
        controls = host.to(dev, non_blocking=False)      # [n, B, n_controls]
        # raw wall forces of every sim step land in one buffer; normalised and averaged once (elementwise division, then the
        # mean over the stack: what torch.stack of the per-step coefficients gave)
        raw = torch.empty(n, self._num_envs, 2, self._ring.nz, dtype=self._dtype, device=dev)
        nu, layer_height = self._wall_force_args()
        for k in range(n):
            self._last_control = controls[k]
            if self._enable_actions:
                self._apply_action(controls[k])
            self._before_sim_step(k)
            self._sim.single_step()
            self._after_sim_step()
            self._ring.forces(self._domain, nu, layer_height=layer_height, out=raw[k])
        self._last_control_mirror = (self._last_control, host[n - 1])
        obs = self._get_global_obs()
        coeff = raw / self._force_norm
        if self._ndims == 2:
            coeff = coeff[..., 0]
        # mean over the sim steps as a loop of adds in step order: `mean(0)` picks its summation order per column, and identical
        # envs of a batch then report drag / lift (hence rewards) that differ in the last bit
        acc = coeff[0].clone()
        for k in range(1, n):
            acc += coeff[k]
        acc /= n
        cd, cl = acc[:, 0], acc[:, 1]
        # 3-D: the reward of the coefficients summed over the span; SpanwiseAgentsMixin divides by D (:765-768)
        reward = self._reward(cd.sum(-1), cl.sum(-1)) if self._ndims == 3 else self._reward(cd, cl)
        return obs, reward, False, {"drag": cd, "lift": cl}

    # ---- on-disk initial domains in the reference's format (fluid_env.py:1044-1112)
    def _save_initial_domain(self, mode, idx: int, env: int = 0) -> None:
        from ..simulation.domain_io import save_multiblock_domain

        out_dir = self._get_domain_dir(idx)
        out_dir.mkdir(parents=True, exist_ok=True)
        save_multiblock_domain(self._domain, str(out_dir / mode.value), env=env, name=self._domain_file_name)

    def load_initial_domain(self, idx: int, mode=None) -> None:
        from pathlib import Path

        from ..simulation.domain_io import load_multiblock_domain

        mode = self._mode if mode is None else mode
        path = self._get_domain_dir(idx) / mode.value
        if not Path(str(path) + ".json").exists():
            return super().load_initial_domain(idx, mode)
        self._pinned_initial = True      # (see FluidEnv.load_initial_domain)
        if self._domain is None:
            self._set_initial_state(randomize=False)
        loaded = load_multiblock_domain(str(path), device=self._cuda_device, batch=self._num_envs)
        try:
            if loaded.n_cells != self._domain.n_cells or [b.size for b in loaded.blocks] != [b.size for b in self._domain.blocks]:
                raise ValueError(f"initial domain {path} does not match this environment's mesh")
            snap = loaded.Clone()
        finally:
            loaded.close()
        self._loaded_initial = snap
        self._domain.Restore(snap)

    def _get_extra_state(self):
        return {"last_control": self._last_control.clone(), "mesh_reset_count": self.mesh_reset_count.copy(),
                "inflow_disturbance": self._inflow_state_dict()}

    def _set_extra_state(self, extra) -> None:
        if extra is not None:
            self._last_control = extra["last_control"].clone()
        self.mesh_reset_count[:] = (extra or {}).get("mesh_reset_count", 0)      # a state from before the counter loads zeros
        self._load_inflow_state((extra or {}).get("inflow_disturbance"))


class SpanwiseAgentsMixin:
    """The multi-agent layer of the 3-D envs (jet_cylinder_env_3d.py:188-480, airfoil_env_3d.py:205-458): the body's span is cut
    into ``_n_segments`` segments with one action each (single agent: all of them; multi-agent: one agent per segment, observing
    ``local_obs_window`` neighbouring segments), the 2-D sensors are stacked on ``_n_sensors_z`` spanwise planes, drag and lift are
    kept per spanwise layer.  A family gives ``_n_segments``, ``_n_sensors_per_agent`` and ``_span_pixel_map``.

    Observation layout: the reference gathers the sensors as ``[z, sensor, component]`` and then *views* that memory as
    ``[z, component, sensor]`` (obs_extraction.py:127-135, ``extract_global_3d_obs``: ``view`` where a ``permute`` was meant), so the
    velocity observation interleaves sensors and components.  Policies trained on the reference see that layout; it is kept (pinned
    on the recorded reference output, tests/test_cylinder_grid.py)."""

    _supports_marl = True
    _n_sensors_per_agent: int

    def _init_spanwise(self, n_segments: int, n_layers: int, local_obs_window: int, use_marl: bool,
                       local_reward_weight: Optional[float], local_2d_obs: bool) -> None:
        """The argument checks and settings of the two 3-D constructors; ``n_layers``: the cell layers along the span."""
        if n_segments < 1 or n_layers % n_segments != 0:
            raise ValueError("n_agents must be a positive integer that evenly divides circle_resolution_angular.")
        if local_2d_obs and not use_marl:
            raise ValueError("Local 2D observations are only supported in multi-agent mode.")
        self._local_2d_obs = bool(local_2d_obs)
        self._nz_per_agent = n_layers // int(n_segments)
        self._local_obs_window = int(local_obs_window)
        self._local_reward_weight = local_reward_weight
        if local_2d_obs:
            self._n_sensors_per_agent = 1
            self._local_obs_window = 1

    @property
    def _n_segments(self) -> int:
        raise NotImplementedError

    def _span_pixel_map(self):
        """``(offset, pixels per unit length)``: a spanwise position z sits on pixel ``round((z + offset) * scale)``."""
        raise NotImplementedError

    def _get_observation_space(self):
        n, spa = self._sensor_locations.shape[-1], self._n_sensors_per_agent
        if self._use_marl and self._local_2d_obs:
            v_shape, p_shape = (n, 2), (n,)
        else:
            lead = self._local_obs_window if self._use_marl else self._n_segments
            v_shape, p_shape = (lead, spa, 3, n), (lead, spa, n)
        return spaces.Dict({
            "velocity": spaces.Box(low=-np.inf, high=np.inf, shape=v_shape, dtype=np.float32),
            "pressure": spaces.Box(low=-np.inf, high=np.inf, shape=p_shape, dtype=np.float32),
        })

    @property
    def n_agents(self) -> int:
        return self._n_segments if self._use_marl else 1

    @property
    def _n_sensors_z(self) -> int:
        return self._n_segments * self._n_sensors_per_agent

    def _get_sensor_locations(self) -> np.ndarray:
        """Pixel (x, y, z) of every sensor, [3, n_sensors_z, n]: the family's 2-D pixels on spanwise planes spread over H."""
        xy = super()._get_sensor_locations()                                     # [2, n]
        nz = self._n_sensors_z
        z = np.linspace(-self.H / 2, self.H / 2, nz + 1, dtype=np.float32)[:-1] + np.float32(self.H / (2 * nz))
        offset, scale = self._span_pixel_map()
        pz = np.round((z + np.float32(offset)) * np.float32(scale)).astype(np.int64)
        out = np.empty((3, nz, xy.shape[1]), np.int64)
        out[0], out[1], out[2] = xy[0][None, :], xy[1][None, :], pz[:, None]
        return out

    # ---- observations (obs_extraction.py:60-205)
    def _get_global_obs(self) -> Dict[str, torch.Tensor]:
        dom = self._domain
        B, nz, n, ns = self._num_envs, self._n_sensors_z, self._sensor_locations.shape[-1], self._n_segments
        u = self._sensors(dom.velocity).to(self._dtype)       # [B, 3, nz * n]
        p = self._sensors(dom.pressure).to(self._dtype)          # [B, nz * n]
        if self._local_2d_obs:
            u = u[:, :2]
        vd = u.shape[1]
        u = u.permute(0, 2, 1).contiguous()                                       # [B, nz * n, vd], as gathered there
        u = u.reshape(B, nz, vd, n).reshape(B, ns, self._n_sensors_per_agent, vd, n)   # the reference's view
        if self._local_2d_obs:
            u = u.permute(0, 1, 2, 4, 3)
        return {"velocity": u, "pressure": p.reshape(B, ns, self._n_sensors_per_agent, n)}

    def _get_local_obs(self) -> Dict[str, torch.Tensor]:
        """Agent a sees the segments a - w//2 ... a + w//2 (periodic): [B, n_agents, window, ...]."""
        g = self._get_global_obs()
        W, ns = self._local_obs_window, self._n_segments
        seg = (torch.arange(ns)[:, None] + torch.arange(W)[None, :] - W // 2) % ns    # [agent, window]
        out = {}
        for k, v in g.items():
            win = v[:, seg.to(v.device)]                                           # [B, ns, W, ...]
            if self._local_2d_obs:
                win = win.reshape(self._num_envs, ns, *win.shape[4:])            # window 1, one sensor layer: squeeze
            out[k] = win
        return out

    # ---- step (jet_cylinder_env_3d.py:427-480, airfoil_env_3d.py:409-458)
    def _step_impl(self, action: torch.Tensor):
        obs, _, term, info = super()._step_impl(action)
        all_cds, all_cls = info.pop("drag"), info.pop("lift")                     # [B, NZ]
        cd, cl = all_cds.sum(-1) / self.D, all_cls.sum(-1) / self.D
        return obs, self._reward(cd, cl), term, {"drag": cd, "lift": cl, "all_cds": all_cds, "all_cls": all_cls}

    def _step_marl_impl(self, actions: torch.Tensor):
        if self._local_reward_weight is None:
            raise ValueError("local_reward_weight must be set for multi-agent step.")
        _, global_reward, terminated, info = self._step_impl(actions)
        local_obs = self._get_local_obs()
        all_cds, all_cls = info.pop("all_cds"), info.pop("all_cls")
        B, ns = self._num_envs, self._n_segments
        local_cd = all_cds.reshape(B, ns, -1).sum(-1) / (self.D / ns)
        local_cl = all_cls.reshape(B, ns, -1).sum(-1) / (self.D / ns)
        w = self._local_reward_weight
        agent_rewards = w * self._reward(local_cd, local_cl) + (1 - w) * global_reward[:, None]
        info["global_reward"] = global_reward
        return local_obs, agent_rewards, terminated, info
