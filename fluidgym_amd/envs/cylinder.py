"""Cylinder (von Karman vortex street) environments on the multi-block HIP path.

Mirrors ``envs/cylinder/cylinder_env_base.py`` (CylinderEnvBase), ``jet_cylinder_env_2d.py`` (CylinderJetEnv2D) and
``rotating_cylinder_env_2d.py`` (CylinderRotEnv2D) of the reference: the same five-block mesh (``cylinder_grid.py``,
pinned on the reference's vertex coordinates), solver settings (:303-329), convective outflow hook (:276-300), 151
velocity / pressure sensors read from the uniformly resampled fields (:430-518), drag / lift by wall-stress integration
(:616-700, ``forces.py``), action smoothing and reward (:741-776).  Batched over ``num_envs`` like every env here.

Not carried over: the published initial domains (HuggingFace ``fluidgym-data``; no network) -- ``reset`` starts from a
projected uniform stream and runs ``initial_domain_steps`` developed-flow steps (the reference generates its initial
domains with 400, :138).  ``_cd_ref`` is the mean drag of the domain statistics once ``compute_domain_statistics`` has written
them, ``drag_reference`` when given, else 0.

``CylinderJetEnv3D`` (``jet_cylinder_env_3d.py``) runs the same mesh extruded over the span (z-periodic): ``n_jets``
spanwise jet segments, 151 x ``n_jets * 2`` sensors read from the 3-D resampled fields, drag / lift per spanwise layer,
single-agent and multi-agent (one agent per segment, windows of neighbouring segments) interfaces.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from ..simulation.multiblock import MultiBlockDomain, MultiBlockSimulation
from .. import spaces
from .channel import jet_profile
from .cylinder_grid import BOTTOM, LEFT, RIGHT, TOP, build_domain, extrude_mesh, make_vortex_street_mesh
from .fluid_env import is_per_env, per_env_parameter, refuse_per_env
from .mesh_body import MeshBodyEnvBase, SpanwiseAgentsMixin

CYLINDER_JET_2D_DEFAULT_CONFIG = {
    "reynolds_number": 1e2, "resolution": 24, "dt": 1e-2, "adaptive_cfl": 0.8, "step_length": 0.25,
    "episode_length": 80, "lift_penalty": 1.0, "use_marl": False, "dtype": torch.float32,
    "load_initial_domain": True, "load_domain_statistics": True, "randomize_initial_state": True,
    "enable_actions": True, "differentiable": False,
}
CYLINDER_ROT_2D_DEFAULT_CONFIG = dict(CYLINDER_JET_2D_DEFAULT_CONFIG)


ONCHIP_PCG_MAX_CELLS = 24 * 1024   # the multilevel-preconditioned on-chip CG (2-D): fg_mb_onchip.hip OC_L2_CELLS

VORTICITY_RENDER_LEVELS = {100: 1.5, 250: 2.5, 500: 3.5}   # jet_cylinder_env_3d.py:15-19: level of the 3-D picture, by Reynolds number


class CylinderEnvBase(MeshBodyEnvBase):
    H: float = 4.1
    D: float = 4.0  # span of the 3-D variants
    L: float = 22.0
    cylinder_diameter: float = 1.0
    _U_mean: float = 1.0
    cylinder_offset_y: float = 0.05
    _n_sensors_x_y: int = 151
    _vortex_street_refinement_base: float = 0.95
    _mesh_reset_sigma = 0.025    # the noise of _randomize_domain, as reset_mesh_envs adds it per env
    _fill_max_steps = 16
    _domain_file_name = "CylinderDomain"

    def __init__(self, reynolds_number: float, resolution: int, dt: float, adaptive_cfl: float, step_length: float,
                 episode_length: int, lift_penalty: float = 1.0, ndims: int = 2, drag_reference: float = 0.0,
                 pressure_use_BiCG=None, **kw):
        if ndims == 3:
            refuse_per_env("reynolds_number", reynolds_number, "the 3-D cylinder env", "per-env parameters are built for the 2-D cylinder envs")
        reynolds_number = per_env_parameter("reynolds_number", reynolds_number, kw.get("num_envs"))      # a number, or one per env
        self._heterogeneous = is_per_env(reynolds_number)
        self._reynolds_number = reynolds_number
        self._circle_resolution_angular = int(resolution)
        self._lift_penalty = lift_penalty
        self._nu = self._U_mean / reynolds_number
        self._drag_reference = float(drag_reference)
        super().__init__(ndims=ndims, pressure_use_BiCG=pressure_use_BiCG, dt=dt, adaptive_cfl=adaptive_cfl, step_length=step_length,
                         episode_length=episode_length, **kw)

    @property
    def _cd_ref(self) -> float:
        """cylinder_env_base.py:270-275: the mean uncontrolled drag of the domain statistics; an explicit non-zero
        ``drag_reference`` wins, and without either it is 0."""
        if self._drag_reference != 0.0:
            return self._drag_reference
        s = self._metric_stat("drag")
        return 0.0 if s is None else float(s.mean)

    def _reward(self, cd: torch.Tensor, cl: torch.Tensor) -> torch.Tensor:
        return self._cd_ref - cd - self._lift_penalty * cl.abs()        # cylinder_env_base.py:765-776

    @property
    def _force_norm(self) -> float:
        return 0.5 * self._U_mean ** 2 * self.cylinder_diameter

    @property
    def _layer_height(self) -> float:
        return self.D / self._circle_resolution_angular      # face area = edge length x D / resolution (:676-689)

    # ---- spaces (cylinder_env_base.py:183-213)
    def _get_action_space(self):
        return spaces.Box(low=-1.0, high=1.0, shape=(1,), dtype=np.float32)

    @property
    def render_shape(self):
        z_res = self._circle_resolution_angular * 4
        return (int(z_res / self.H * self.L), z_res, z_res)

    @property
    def id(self) -> str:
        self._refuse_heterogeneous_id()
        return f"{type(self).__name__}_Re{self._reynolds_number}"

    @property
    def initial_domain_id(self) -> str:
        self._refuse_heterogeneous_id()
        return f"cylinder_{self._ndims}D_Re{int(self._reynolds_number)}_Res{self._circle_resolution_angular}"

    # ---- sensors (cylinder_env_base.py:430-518)
    def _get_sensor_locations_2d(self) -> np.ndarray:
        xs, ys = np.arange(1.0, 5.0, 0.5), np.arange(-1.5, 1.75, 0.5)
        gx, gy = np.meshgrid(xs, ys, indexing="ij")
        main = np.stack([gx.ravel(), gy.ravel()])
        x1 = np.arange(-0.25, 1, 0.25)
        x2 = np.concatenate([[-0.25], np.arange(0.25, 1.25, 0.25)])
        x3 = np.array([0.75] * 3)
        extra = np.stack([np.concatenate([x1, x1, x2, x2, x3]),
                          np.concatenate([np.full_like(x1, -1.5), np.full_like(x1, 1.5), np.full_like(x2, self.cylinder_diameter),
                                          np.full_like(x2, -self.cylinder_diameter), np.array([-0.5, 0, 0.5])])])
        ang = np.linspace(0, 2 * np.pi, 36).astype(np.float32)  # float32 like the reference's torch.linspace: the sensor at
        c1 = np.float32(1.0) * np.stack([np.cos(ang), np.sin(ang)])   # angle 2 pi sits on a rounding tie of the pixel grid
        c2 = np.float32(0.625) * np.stack([np.cos(ang), np.sin(ang)])
        return np.concatenate([main.astype(np.float32), c1, c2, extra.astype(np.float32)], axis=1).astype(np.float32)

    def _get_sensor_locations(self) -> np.ndarray:
        """Pixel (x, y) of every sensor in the resampled field (``_sensor_locations_to_grid_coords``)."""
        p = self._get_sensor_locations_2d().copy()
        p[0] = (p[0] + np.float32(2.0)) * np.float32((self.render_shape[0] - 1) / (self.L - 2.0))
        p[1] = (p[1] + np.float32(self.H / 2)) * np.float32((self.render_shape[1] - 1) / self.H)
        return np.round(p).astype(np.int64)

    # ---- domain and simulation (cylinder_env_base.py:233-329)
    def _get_domain(self) -> MultiBlockDomain:
        self._mesh = make_vortex_street_mesh(self._circle_resolution_angular, self.H, self.L, self.cylinder_diameter / 2,
                                             self.cylinder_offset_y, self.cylinder_diameter / 2, self.cylinder_diameter,
                                             self._vortex_street_refinement_base)
        if self._ndims == 3:   # grid.py:281-294: res_z = resolution, z in [-2, 2]
            self._mesh = extrude_mesh(self._mesh, self._circle_resolution_angular, -self.D / 2, self.D / 2)
        # dtype=torch.float64: the fp64 build of the multi-block path (plain recurrences, one cell per thread; observations are
        # resampled in float32 and handed back in the env's dtype)
        return build_domain(self._mesh, self._nu, batch=self._num_envs, device=self._cuda_device,
                            non_ortho_flags=self._non_ortho_flags, dtype=self._dtype)

    def _get_simulation(self, domain, prep_fn):
        # solver policy pressure_bicgstab_large_meshes: beyond the preconditioned on-chip CG's reach (2-D meshes of up to 24 576 cells:
        # every 2-D id; csrc/fg_mb_onchip.hip k_mbc_onchip / k_mbc_l2) the pressure systems go to the fp64-refined BiCGStab unless
        # the caller chose (policy.py)
        from ..simulation.policy import get_solver_policy
        if self._pressure_use_bicg is None:     # (None = not chosen by the caller; False = the reference's CG, 1 / 2 = BiCGStab / refined)
            self._pressure_use_bicg = 2 if (get_solver_policy()["pressure_bicgstab_large_meshes"]
                                            and (self._ndims == 3 or domain.n_cells > ONCHIP_PCG_MAX_CELLS)) else False
        sim = MultiBlockSimulation(domain, dt=self._dt, adaptive_CFL=self._adaptive_cfl, substeps="ADAPTIVE", corrector_steps=2,
                                   pressure_tol=1e-5 if self._ndims == 2 else 5e-7, advect_non_ortho_steps=1,
                                   pressure_non_ortho_steps=1 if self._ndims == 2 else 4,
                                   pressure_use_BiCG=self._pressure_use_bicg, outflow=self._mesh.outflow,
                                   outflow_velocity=(self._U_mean, 0.0, 0.0), outflow_tol=5e-6,
                                   solver_double_fallback=True, BiCG_precondition_fallback=True)   # cylinder_env_base.py:326-328
        return sim

    def _wall_ring_segments(self) -> list:
        return [(LEFT, "+x", False), (TOP, "-y", False), (RIGHT, "-x", True), (BOTTOM, "+y", True)]

    def _use_pressure_multilevel(self) -> bool:
        from ..simulation.policy import get_solver_policy
        return bool(get_solver_policy()["pressure_multilevel"] and not self._pressure_deflation and not self._pressure_use_bicg)

    def _mesh_reset_warmup_env_steps(self) -> int:
        """Two shedding periods (cylinder_env_base.py:364-404)."""
        period = 1.0 / (0.3 * self._U_mean / self.cylinder_diameter)
        return 2 * int(period / self._step_length) - 1

    def _get_cylinder_mask(self) -> np.ndarray:
        """Pixels ``[ny, nx]`` (3-D: repeated along z, ``[nz, ny, nx]``) inside the cylinder on the render grid
        (cylinder_env_base.py:518-535)."""
        nx, ny = self.render_shape[0], self.render_shape[1]
        radius = self.cylinder_diameter / 2 * (ny - 1) / self.H
        center_x = round((nx - 1) / self.L * 2.0)
        center_y = round((ny - 1) / self.H * 2.0)
        Y, X = np.ogrid[:ny, :nx]
        mask = np.sqrt((X - center_x) ** 2 + (Y - center_y) ** 2) <= radius
        if self._ndims == 3:
            mask = np.repeat(mask[None, :, :], self.render_shape[2], axis=0)
        return mask

    def _frame_specs(self):
        """cylinder_env_base.py:700-739: vorticity in (-10, 10), ``icefire``, the cylinder black.  The mask slices are the
        reference's: ``[y, x]``; in 3-D ``mask[0]``, ``mask[:, 0, :]`` and ``mask[:, :, 0]`` (the last two hold no solid pixel; the
        third is ``[z, y]`` laid over the ``[y, z]`` frame, which the render grid's equal y and z extents allow there and here)."""
        m = self.__dict__.get("_cylinder_mask")
        if m is None:
            m = self._cylinder_mask = self._get_cylinder_mask()
        if self._ndims == 2:
            masks = (self._frame_mask("xy", m),)
        else:
            masks = (self._frame_mask("xy", m[0]), self._frame_mask("xz", m[:, 0, :]), self._frame_mask("yz", m[:, :, 0]))
        return self._vortex_frame_specs((-10, 10), False, masks)

    def _frame_specs_3d(self):
        m = self.__dict__.get("_cylinder_mask")
        if m is None:
            m = self._cylinder_mask = self._get_cylinder_mask()
        return self._vortex_frame_specs_3d(VORTICITY_RENDER_LEVELS, 20, self._frame_mask("xyz", m), (self.L, self.H, self.H))


def _face_vertices(mesh, block: int, face: str) -> np.ndarray:
    c = mesh.coords[block].astype(np.float64)
    if c.shape[0] == 3:
        c = c[:2, 0]          # the first spanwise layer ("we set z = 0", jet_cylinder_env_3d.py:378-381)
    return {"+x": c[:, :, -1], "-x": c[:, :, 0], "-y": c[:, 0, :], "+y": c[:, -1, :]}[face]


class CylinderJetEnv2D(CylinderEnvBase):
    """Two synthetic jets at the poles of the cylinder, blowing / sucking with zero net mass flux
    (jet_cylinder_env_2d.py:124-186)."""

    _jet_angle: float = 10.0  # degrees

    def _jet_velocities(self, boundary_vertices: np.ndarray, top: bool) -> np.ndarray:
        centers = 0.5 * (boundary_vertices[:, :-1] + boundary_vertices[:, 1:])
        base = np.pi / 2 if top else -np.pi / 2
        deg = np.rad2deg(base - np.arctan2(centers[1], centers[0]))
        mag = np.abs(deg)
        mag[mag > self._jet_angle] = 0.0
        nz = np.nonzero(mag > 0.0)[0]
        lo, hi = nz[0] - 1, nz[-1] + 1
        prof = jet_profile(int(hi - lo + 1))
        vel = np.zeros_like(centers)
        for i, u in zip(range(lo, hi + 1), prof):
            vel[0, i] = u * np.sin(np.deg2rad(deg[i]))
            vel[1, i] = u * np.cos(np.deg2rad(deg[i]))
        return vel.astype(np.float32)

    def _additional_initialization(self) -> None:
        super()._additional_initialization()
        dev = self._domain.device
        self._top_velocity = torch.as_tensor(self._jet_velocities(_face_vertices(self._mesh, TOP, "-y"), True), device=dev).to(self._dtype)
        self._bottom_velocity = torch.as_tensor(self._jet_velocities(_face_vertices(self._mesh, BOTTOM, "+y"), False), device=dev).to(self._dtype)

    def _apply_action(self, action: torch.Tensor) -> None:
        a = action.reshape(self._num_envs, 1, 1)
        dom = self._domain
        # written straight into the boundary slots (one launch per jet instead of a product and a copy)
        torch.mul(self._top_velocity[None], a, out=dom.blocks[TOP].boundary("-y"))
        torch.mul(self._bottom_velocity[None], a, out=dom.blocks[BOTTOM].boundary("+y"))


def rotating_wall_velocities(mesh):
    """Unit tangential velocity on the cylinder-wall faces of the four blocks around it, ``[(block, face, [2, n_faces])]``
    (rotating_cylinder_env_2d.py:131-164)."""
    out = []
    for b, face in ((LEFT, "+x"), (TOP, "-y"), (RIGHT, "-x"), (BOTTOM, "+y")):
        v = _face_vertices(mesh, b, face)
        ctr = 0.5 * (v[:, :-1] + v[:, 1:])
        th = np.arctan2(ctr[1], ctr[0])
        out.append((b, face, np.stack([np.sin(th), -np.cos(th)]).astype(np.float32)))
    return out


class CylinderRotEnv2D(CylinderEnvBase):
    """The cylinder wall rotates with the commanded speed (rotating_cylinder_env_2d.py:121-176)."""

    def _additional_initialization(self) -> None:
        super()._additional_initialization()
        dev = self._domain.device
        self._wall = [(b, face, torch.as_tensor(v, device=dev).to(self._dtype)) for b, face, v in rotating_wall_velocities(self._mesh)]

    def _apply_action(self, action: torch.Tensor) -> None:
        a = action.reshape(self._num_envs, 1, 1)
        for b, face, vel in self._wall:
            torch.mul(vel[None], a, out=self._domain.blocks[b].boundary(face))


CYLINDER_JET_3D_DEFAULT_CONFIG = {
    "n_jets": 8, "reynolds_number": 1e2, "resolution": 24, "dt": 1e-2, "adaptive_cfl": 0.8, "step_length": 0.25,
    "lift_penalty": 1.0, "episode_length": 80, "local_obs_window": 3, "local_reward_weight": 0.8, "local_2d_obs": False,
    "use_marl": False, "dtype": torch.float32, "load_initial_domain": True, "load_domain_statistics": True,
    "randomize_initial_state": True, "enable_actions": True, "differentiable": False,
}


class CylinderJetEnv3D(SpanwiseAgentsMixin, CylinderJetEnv2D):
    """``CylinderJetEnv3D`` (jet_cylinder_env_3d.py:44-480): the cylinder spans z in [-2, 2] (periodic), the two jet slots
    are cut into ``n_jets`` spanwise segments, each driven by one action; observations, agents and per-layer forces are
    ``mesh_body.SpanwiseAgentsMixin``."""

    _n_sensors_per_agent: int = 2

    def __init__(self, n_jets: int, reynolds_number: float, resolution: int, dt: float, adaptive_cfl: float,
                 step_length: float, episode_length: int, lift_penalty: float, local_obs_window: int, use_marl: bool,
                 local_reward_weight: Optional[float], local_2d_obs: bool = False, **kw):
        self._init_spanwise(n_jets, resolution, local_obs_window, use_marl, local_reward_weight, local_2d_obs)
        self._n_jets = int(n_jets)
        self._n_controls = self._n_jets
        kw.pop("ndims", None)
        super().__init__(reynolds_number=reynolds_number, resolution=resolution, dt=dt, adaptive_cfl=adaptive_cfl,
                         step_length=step_length, episode_length=episode_length, lift_penalty=lift_penalty, ndims=3,
                         use_marl=use_marl, **kw)

    @property
    def _n_segments(self) -> int:
        return self._n_jets

    def _span_pixel_map(self):
        """The spanwise sensor planes are spread over H (not D) and scaled with the y resolution, as in the reference
        (jet_cylinder_env_3d.py:277-304; cylinder_env_base.py:436-449)."""
        return self.H / 2, (self.render_shape[1] - 1) / self.H

    # ---- spaces (jet_cylinder_env_3d.py:188-258)
    def _get_action_space(self):
        shape = (1,) if self._use_marl else (self._n_jets, 1)
        return spaces.Box(low=-1.0, high=1.0, shape=shape, dtype=np.float32)

    @property
    def id(self) -> str:
        return f"JetCylinder3D_Re{self._reynolds_number}"

    # ---- actuation (jet_cylinder_env_3d.py:341-421)
    def _additional_initialization(self) -> None:
        super()._additional_initialization()
        nz = self._circle_resolution_angular
        z3 = lambda v: torch.cat([v, torch.zeros_like(v[:1])], dim=0)[:, None, :].expand(3, nz, v.shape[1])
        self._top_velocity3 = z3(self._top_velocity).contiguous()                 # [3, nz, nx]
        self._bottom_velocity3 = z3(self._bottom_velocity).contiguous()

    def _apply_action(self, action: torch.Tensor) -> None:
        """One amplitude per spanwise segment, repeated over the segment's layers.  (The reference then rebalances the
        boundary fluxes over both jet faces and the outflow with tol 1e-7; the jets are flux-neutral by construction and
        the outflow is rebalanced by every step's PRE hook here, so that call is not repeated.)"""
        B = self._num_envs
        a = action.reshape(B, self._n_jets).repeat_interleave(self._nz_per_agent, dim=1)[:, None, :, None]   # [B, 1, nz, 1]
        dom = self._domain
        dom.blocks[TOP].boundary("-y").copy_((self._top_velocity3[None] * a).reshape(B, 3, -1))
        dom.blocks[BOTTOM].boundary("+y").copy_((self._bottom_velocity3[None] * a).reshape(B, 3, -1))
