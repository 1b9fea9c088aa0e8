"""``probe`` and ``start_tracers`` / ``stop_tracers`` of the single-block envs (RBC, TCF, channel): field values at physical
positions, and a cloud of Lagrangian tracers (``simulation/tracers.TracerCloud``) that is advected on the GPU after every
``every``-th sim step of ``step()`` while it is active.  ``reset()`` returns every env's tracers to their seeds, ``reset_envs(envs)``
those of the chosen envs and no other; ``get_state()`` carries the cloud under the key ``"tracers"`` while one is active and
``set_state()`` restores it.  Without an active cloud the step, reset and state paths do nothing for the tracers."""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from ..simulation.domain import Domain
from ..simulation.tracers import PointGrid, TracerCloud


class TracerMixin:
    _tracers: Optional[TracerCloud] = None          # None (the default): the step path does nothing for the tracers
    _tracers_every: int = 1
    _tracers_tick: int = 0
    _probe_grid: Optional[PointGrid] = None

    def _require_single_block(self, entry: str) -> None:
        if getattr(self, "_domain", None) is None:
            raise RuntimeError(f"{entry}: reset() the env first (the domain does not exist yet)")
        if not isinstance(self._domain, Domain):
            raise NotImplementedError(f"{entry} needs a single-block domain (RBC, TCF, channel envs); it is not implemented for "
                                      "multi-block envs (cylinder, airfoil)")

    @property
    def tracers(self) -> Optional[TracerCloud]:
        """The active cloud, or None."""
        return self._tracers

    def probe(self, points, fields: Optional[Sequence[str]] = None) -> torch.Tensor:
        """``fields`` (default ``u, v(, w), p(, T)``) at the physical positions ``points`` (``[P, d]`` for every env, or
        ``[B, P, d]``) in every env: ``[B, P, K]`` on the GPU, one launch."""
        self._require_single_block("probe")
        if self._probe_grid is None or self._probe_grid.domain is not self._domain:
            self._probe_grid = PointGrid(self._domain)
        return self._probe_grid.sample(points, fields)

    def _tracer_respawn_faces(self) -> tuple:
        """The FIXED faces beyond which a tracer returns to its seed (an env with an inflow and an outflow names them).  Default: none."""
        return ()

    def start_tracers(self, n: int, seed: Optional[int] = None, positions=None, substeps: int = 4, every: int = 1) -> TracerCloud:
        """Start a fresh cloud of ``n`` tracers per env (``TracerCloud``: ``seed`` or ``positions``); after every ``every``-th sim step
        of ``step()`` it is advanced by ``every`` sim time steps in the velocity field of that moment."""
        self._require_single_block("start_tracers")
        if int(every) < 1:
            raise ValueError(f"every must be at least 1, got {every}")
        self._tracers = TracerCloud(self._domain, n, seed=seed, positions=positions, substeps=substeps,
                                    respawn_faces=self._tracer_respawn_faces())
        self._tracers_every, self._tracers_tick = int(every), 0
        return self._tracers

    def stop_tracers(self) -> TracerCloud:
        """Stop advecting and hand out the cloud."""
        self._require_single_block("stop_tracers")
        if self._tracers is None:
            raise RuntimeError("stop_tracers: no tracers are active")
        cloud, self._tracers = self._tracers, None
        return cloud

    def _sim_step_time(self) -> float:
        sim = self._sim
        return float(sim.time_step if sim.substeps == -1 else sim.time_step * max(sim.substeps, 1))

    def _advect_tracers(self) -> None:
        """Called after a sim step while a cloud is active."""
        self._tracers_tick += 1
        if self._tracers_tick % self._tracers_every == 0:
            self._tracers.advect(self._tracers_every * self._sim_step_time())

    def _tracer_state(self) -> dict:
        return {"cloud": self._tracers.state_dict(), "every": self._tracers_every, "tick": self._tracers_tick}

    def _set_tracer_state(self, state: dict) -> None:
        if self._tracers is None:
            raise RuntimeError("set_state: the state holds a tracer cloud but none is active; call start_tracers() with its size first")
        self._tracers.load_state_dict(state["cloud"])
        self._tracers_every, self._tracers_tick = int(state["every"]), int(state["tick"])
