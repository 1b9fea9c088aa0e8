"""The two classical baseline controllers of the benchmarks, computed on the GPU for the whole batch.

The reference's documentation promises both (``docs/source/api/tcf.rst``: opposition control, ``v_wall = -alpha v'(x, y+ = 15, z)`` with
``alpha = 1``; the RBC pages: a PD controller ``a = k_p E + k_d dE/dt`` with ``k_p = 970``, ``k_d = 2000``) and carries the containers
(``TCF3DBottomEnv.scale_actions``, ``save_opposition_control_episode``), but ships no controller code.  Here an action of the whole batch
is ONE launch of ``fg_baseline_opposition`` / ``fg_baseline_pd`` (``csrc/fg_baselines.hip``) on the current stream: fp64 sums in a fixed
order, so identical envs get bit-identical actions and nothing returns to the host.

``run_baseline_episodes`` steps an env with a controller and hands back one ``pandas.DataFrame`` per env of the batch -- for the channel
the frames ``save_opposition_control_episode`` takes.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional

import numpy as np
import torch

from . import _lib as L
from .simulation import plane_fields as F


def _bound_block(env, who: str):
    """The block of a reset env (the fields exist from the first ``reset()`` on)."""
    if getattr(env, "_domain", None) is None:
        raise RuntimeError(f"{who}: the environment has no state yet. Call 'reset()' first.")
    return env._block


def _velocity(block) -> torch.Tensor:
    """The block's velocity ``[B, d, (Z,) Y, X]``; the kernels read component 1 in place (its pointer in env 0, the batch stride
    ``d`` fields)."""
    u = block.velocity
    if not u.is_contiguous():
        raise RuntimeError("the block's velocity must be contiguous")
    return u


class OppositionControl:
    """Opposition control of ``TCF3DBottomEnv`` / ``TCF3DBothEnv`` (Choi, Moin & Kim 1994): every actuator blows against the
    wall-normal velocity fluctuation ``v' = v - <v>_{z,x}`` it sees on the detection plane, ``v_wall = -alpha v'``, averaged over its
    ``actor_size x actor_size`` patch.

    Detection rows: at the bottom wall the cell layer whose centre is nearest ``y+ = y_plus`` (at 15 the env's own
    ``_y_obs_bottom_idx``); at the top wall its true mirror ``ny - 1 - idx`` -- not the ``ny - idx`` of the env's top observation,
    which is off by one on purpose (``tcf.py``, ``_y_obs_top_idx``): the controller is symmetric by construction.  Gains
    ``(-alpha, +alpha)``: the env negates the top wall's control itself (``TCF3DBothEnv._apply_action``), so both walls end up at
    ``v_wall = -alpha v'``.

    ``action()`` returns a tensor in the shape of ``env.sample_action()`` (single- and multi-agent alike), ready for ``env.step``.  It
    raises ``RuntimeError`` while ``env.scale_actions`` is true: shifted, clamped and scaled by ``u_tau`` it would not be opposition
    control."""

    def __init__(self, env, alpha: float = 1.0, y_plus: float = 15.0):
        from .envs.tcf import TCF3DBothEnv, TCF3DBottomEnv

        if not isinstance(env, TCF3DBottomEnv):
            raise TypeError(f"OppositionControl drives the turbulent-channel envs (TCF3DBottomEnv, TCF3DBothEnv), not {type(env).__name__}")
        self.env, self.alpha, self.y_plus = env, float(alpha), float(y_plus)
        self.n_walls = 2 if isinstance(env, TCF3DBothEnv) else 1
        self._rows = None

    def detection_rows(self) -> List[int]:
        """``[bottom]`` or ``[bottom, top]`` cell rows of the detection planes."""
        if self._rows is None:
            e = np.asarray(_bound_block(self.env, "OppositionControl").edges[1], np.float64)
            ycen = 0.5 * (e[1:] + e[:-1])
            idx = int(np.abs(ycen - self.env._y_wall_to_y(self.y_plus)).argmin())
            self._rows = [idx, len(ycen) - 1 - idx][: self.n_walls]
        return list(self._rows)

    def action(self) -> torch.Tensor:
        env = self.env
        if env.scale_actions:
            raise RuntimeError("OppositionControl.action: env.scale_actions is True; scaled actions are not opposition control. "
                               "Set env.scale_actions = False (run_baseline_episodes does).")
        u = _velocity(_bound_block(env, "OppositionControl.action"))
        B, nz, ny, nx = F.grid_of(u)
        actor, W = env._actor_size, self.n_walls
        rows = (ctypes.c_int32 * W)(*self.detection_rows())
        gain = (ctypes.c_double * W)(*[-self.alpha, self.alpha][:W])
        out = torch.empty(B, W, nx // actor, nz // actor, dtype=u.dtype, device=u.device)
        cells = nz * ny * nx
        lib = F.library(u.dtype)
        with torch.cuda.device(u.device):
            L.check(lib.fg_baseline_opposition(ctypes.c_void_p(u.data_ptr() + cells * u.element_size()), int(u.shape[1]) * cells, B, nz, ny, nx,
                                               rows, gain, W, actor, F.ptr(out), F.stream_ptr(u.device)), lib=lib)
        return out.reshape(env._zero_action.shape)


class PDControl:
    """PD control of the Rayleigh-Benard envs, 2-D and 3-D: per heater ``E`` = the vertical velocity averaged over the fluid column
    above it (over the heater's cells in x (and z), weighted by the cell heights ``wy`` along y), and
    ``action = -(kp E + kd (E - E_previous) / dt)`` with ``dt = env.step_length``.

    The minus sign is this package's decision: ``E`` is the UPWARD velocity, the action raises the heater's temperature, and a
    positive gain must cool under a rising plume to damp it.  The reference documents the gains (``k_p = 970``, ``k_d = 2000``) but
    ships no controller code that would pin the sign of its ``E``.

    The derivative term is zero at the first ``action()`` and at the first one after ``reset()`` -- for all envs, or for the named
    ones, so that it composes with ``env.reset_envs(envs)``.  The state (``E`` of the previous call and the per-env ``first`` flag)
    lives on the device; ``action()`` is one launch and returns a tensor in the shape of ``env.sample_action()``."""

    def __init__(self, env, kp: float = 970.0, kd: float = 2000.0):
        from .envs.rbc import RBCEnvBase

        if not isinstance(env, RBCEnvBase):
            raise TypeError(f"PDControl drives the Rayleigh-Benard envs (RBCEnv2D, RBCEnv3D), not {type(env).__name__}")
        self.env, self.kp, self.kd = env, float(kp), float(kd)
        self._state = None          # (wy [ny] fp64, e_state [B, nhz, nhx] fp64, first [B] int32, tickets [B] int64) on the device

    def _bind(self):
        if self._state is None:
            env = self.env
            blk = _bound_block(env, "PDControl")
            dev = blk.velocity.device
            B, nz, ny, nx = F.grid_of(blk.velocity)
            seg = env._heater_width
            h = np.diff(np.asarray(blk.edges[1], np.float64))
            self._state = (torch.as_tensor(h / h.sum(), dtype=torch.float64, device=dev),
                           torch.zeros(B, nz // seg if nz > 1 else 1, nx // seg, dtype=torch.float64, device=dev),
                           torch.ones(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int64, device=dev))
        return self._state

    def reset(self, envs=None) -> None:
        """Forget the previous ``E`` of all envs (``envs=None``) or of the envs ``envs`` (indices or a bool mask ``[num_envs]``):
        their next action has no derivative term."""
        if self._state is None and getattr(self.env, "_domain", None) is None:
            return                  # nothing recorded yet: the first action of every env has no derivative term anyway
        first = self._bind()[2]
        if envs is None:
            first.fill_(1)
        else:
            from .simulation.state_bank import normalize_envs

            first[torch.as_tensor(normalize_envs(envs, int(first.numel())), dtype=torch.int64, device=first.device)] = 1

    def action(self) -> torch.Tensor:
        env = self.env
        wy, e_state, first, tickets = self._bind()
        u = _velocity(_bound_block(env, "PDControl.action"))
        B, nz, ny, nx = F.grid_of(u)
        out = torch.empty(e_state.shape, dtype=u.dtype, device=u.device)
        cells = nz * ny * nx
        lib = F.library(u.dtype)
        with torch.cuda.device(u.device):
            L.check(lib.fg_baseline_pd(ctypes.c_void_p(u.data_ptr() + cells * u.element_size()), int(u.shape[1]) * cells, B, nz, ny, nx,
                                       env._heater_width, F.ptr(wy), self.kp, self.kd / float(env.step_length), F.ptr(e_state),
                                       F.ptr(first), F.ptr(tickets), F.ptr(out), F.stream_ptr(u.device)), lib=lib)
        return out.reshape(env._zero_action.shape)


def run_baseline_episodes(env, controller, seed: int, steps: Optional[int] = None, randomize: Optional[bool] = None):
    """``env.reset(seed, randomize)``, then ``steps`` env steps (default ``env.episode_length``) with ``controller.action()``.  For an
    ``OppositionControl`` the env's ``scale_actions`` is switched off for the run and put back afterwards.  Returns one
    ``pandas.DataFrame`` per env of the batch with the columns ``step``, ``reward`` (the mean over the agents of a multi-agent env) and
    every key of ``info``; the series stay on the device until the run is over.  For the channel envs these are the frames
    ``save_opposition_control_episode`` takes."""
    import pandas as pd

    n = int(env.episode_length if steps is None else steps)
    if n < 1:
        raise ValueError("steps must be at least 1")
    B = env.num_envs
    opposition = isinstance(controller, OppositionControl)
    env.reset(seed=seed, randomize=randomize)
    if hasattr(controller, "reset"):
        controller.reset()
    if opposition:
        scaled, env.scale_actions = env.scale_actions, False
    series = {}
    try:
        for _ in range(n):
            _, reward, _, _, info = env.step(controller.action())
            for key, value in (("reward", reward), *info.items()):
                series.setdefault(key, []).append(torch.as_tensor(value).detach().reshape(B, -1).to(torch.float64).mean(dim=1))
    finally:
        if opposition:
            env.scale_actions = scaled
    host = {key: torch.stack(v).cpu().numpy() for key, v in series.items()}              # [steps, B] each
    return [pd.DataFrame({"step": np.arange(n), **{key: v[:, b] for key, v in host.items()}}) for b in range(B)]
