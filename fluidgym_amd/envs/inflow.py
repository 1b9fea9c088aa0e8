"""Per-env unsteady inflow -- gusts -- on the multi-block envs (cylinder, airfoil).  While a disturbance is active, every
sim step of ``step()`` is preceded by ONE launch (``MultiBlockDomain.ApplyInflowDisturbance``) that rewrites the inflow face of every
env from the steady profile (``_initial_boundary``) and that env's gust signals, and rescales the outflow so that the boundary
fluxes balance again, which the guard at the top of the native step asks.  The time of env b is ``(episode_steps[b] * n_sim_steps + k)
* dt`` and its episode ``mesh_reset_count[b]``: ``reset_mesh_envs`` gives the chosen envs new modes and t = 0 and leaves the others
alone, ``reset(seed=...)`` starts every env at episode 0, and ``get_state()`` / ``set_state()`` carry the description beside the last
control (the counters travel already).  Nothing is remembered between launches.

Only ``step()`` is disturbed.  The development of the initial fields, ``_randomize_domain``, ``record_mesh_state_bank`` and
``compute_domain_statistics`` call ``sim.single_step()`` directly and see the boundary values as they stand (the steady profile unless
a disturbance is active, then the last gust, frozen).  This is not a step hook: it runs BEFORE the sim step and is no part of
``HOOK_ORDER``."""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from ..simulation.inflow_disturbance import InflowDisturbance


class InflowDisturbanceMixin:
    _inflow_spec: Optional[InflowDisturbance] = None
    _inflow_signal: Optional[torch.Tensor] = None
    _inflow_counters: Optional[torch.Tensor] = None

    @property
    def inflow_disturbance(self) -> Optional[InflowDisturbance]:
        """The active ``InflowDisturbance`` (None: the steady inflow)."""
        return self._inflow_spec

    def _inflow_counter_words(self) -> np.ndarray:
        """``[B, 2]`` = (env steps of env b's episode, env b's episode) as the 32-bit words the kernel reads."""
        c = np.stack([np.asarray(self.episode_steps, dtype=np.int64), np.asarray(self.mesh_reset_count, dtype=np.int64)], axis=1)
        return (c & 0xFFFFFFFF).astype(np.uint32)

    def _require_inflow(self, entry: str) -> None:
        if not self._reset_called or self._domain is None:
            raise RuntimeError(f"Environment must be reset before {entry}(). Call 'reset()' first.")

    def start_inflow_disturbance(self, spec: Optional[InflowDisturbance] = None, **random_kwargs) -> InflowDisturbance:
        """Install an ``InflowDisturbance``, or the random form built from ``random_kwargs`` (``seed``, ``n_streamwise``,
        ``n_transverse``, ``band``, ``streamwise_rms``, ``transverse_rms``, ``kappa``, ``env_offset``); it acts from the next
        ``step()``.  The face centres of the inflow face are uploaded once (3-D: repeated along z, so the gust is uniform over the
        span)."""
        self._require_inflow("start_inflow_disturbance")
        if (spec is None) == (not random_kwargs):
            raise ValueError("start_inflow_disturbance: an InflowDisturbance, or the keyword arguments of InflowDisturbance.random")
        if spec is None:
            spec = InflowDisturbance.random(**random_kwargs)
        if not isinstance(spec, InflowDisturbance):
            raise TypeError("start_inflow_disturbance: spec must be an InflowDisturbance")
        return self._install_inflow(spec)

    def _install_inflow(self, spec: InflowDisturbance) -> InflowDisturbance:
        spec.modes_table(self._num_envs)          # (a table for another batch refuses here)
        dev = self._domain.device
        self._inflow_spec = spec
        self._inflow_signal = torch.zeros(self._num_envs, 2, dtype=torch.float32, device=dev)
        self._inflow_counters = torch.zeros(self._num_envs, 2, dtype=torch.int32, device=dev)
        return spec

    def _inflow_launch(self, spec, k: int) -> None:
        sim = self._sim
        self._domain.ApplyInflowDisturbance(self._mesh.inflow, sim.outflow, self._initial_boundary, spec, self._n_sim_steps, k,
                                            self._inflow_counters, sim.time_step, outflow_tol=sim.outflow_tol, signal=self._inflow_signal)

    def stop_inflow_disturbance(self) -> None:
        """Write the steady profile back and rebalance the outflow (one launch at zero amplitude), then remove the disturbance."""
        if self._inflow_spec is None:
            raise RuntimeError("stop_inflow_disturbance: no inflow disturbance is active")
        self._inflow_launch(None, 0)
        self._inflow_spec = self._inflow_signal = self._inflow_counters = None

    def inflow_signal(self) -> torch.Tensor:
        """``[B, 2]`` fp32: (S_b, G_b at the mid-height of the inflow face) of the last sim step."""
        if self._inflow_spec is None:
            raise RuntimeError("inflow_signal: no inflow disturbance is active")
        return self._inflow_signal.clone()

    def _before_sim_step(self, k: int) -> None:
        """Called by the sim-step loops right before ``sim.single_step()`` with the index of the sim step within the env step."""
        if self._inflow_spec is None:
            return
        if k == 0:      # the one upload of an env step: where every env stands in its episode
            words = torch.from_numpy(self._inflow_counter_words().view(np.int32))
            self._inflow_counters.copy_(words, non_blocking=False)
        self._inflow_launch(self._inflow_spec, k)

    def step(self, action: torch.Tensor):
        obs, reward, terminated, truncated, info = super().step(action)
        if self._inflow_spec is not None:
            info["inflow"] = self._unbatch(self._inflow_signal.clone())
        return obs, reward, terminated, truncated, info

    # ---- the description travels beside the last control (MeshBodyEnvBase._get_extra_state / _set_extra_state)
    def _inflow_state_dict(self) -> Optional[dict]:
        return None if self._inflow_spec is None else self._inflow_spec.state_dict()

    def _load_inflow_state(self, d: Optional[dict]) -> None:
        if d is None:
            self._inflow_spec = self._inflow_signal = self._inflow_counters = None
        else:
            self._install_inflow(InflowDisturbance.from_state_dict(d))
