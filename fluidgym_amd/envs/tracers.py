"""``probe`` and ``start_tracers`` / ``stop_tracers`` of the single-block envs (RBC, TCF, channel): field values at physical
positions, and a cloud of Lagrangian tracers (``simulation/tracers.TracerCloud``) that is advected on the GPU after every
``every``-th sim step of ``step()`` while it is active.  ``reset()`` returns every env's tracers to their seeds, ``reset_envs(envs)``
those of the chosen envs and no other; ``get_state()`` carries the cloud under the key ``"tracers"`` while one is active and
``set_state()`` restores it.  An active cloud is one entry of the env's hook list (``envs/step_hooks.py``), which does all of that;
without one the step, reset and state paths do nothing for the tracers."""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from ..simulation.domain import Domain
from ..simulation.tracers import PointGrid, TracerCloud


class TracerMixin:
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
        return self._hook("tracers")

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
        cloud = TracerCloud(self._domain, n, seed=seed, positions=positions, substeps=substeps, respawn_faces=self._tracer_respawn_faces())
        # (the interval reads the hook's own ``every``: set_state() may have restored another one)
        return self._start_hook("tracers", cloud, every, lambda: cloud.advect(self._step_hooks["tracers"].every * self._sim_step_time()),
                                reseed=cloud.reseed, state_key="tracers")

    def stop_tracers(self) -> TracerCloud:
        """Stop advecting and hand out the cloud."""
        self._require_single_block("stop_tracers")
        return self._stop_hook("tracers", "stop_tracers: no tracers are active")

    def _sim_step_time(self) -> float:
        sim = self._sim
        return float(sim.time_step if sim.substeps == -1 else sim.time_step * max(sim.substeps, 1))


class MeshTracerMixin:
    """``locate_probes`` and ``start_mesh_tracers`` / ``stop_mesh_tracers`` of the multi-block envs (cylinder, airfoil): point probes at
    physical positions of the curvilinear mesh, located once and sampled in one launch (``simulation/mb_tracers.MeshProbes``), and a
    cloud of Lagrangian tracers (``MeshTracerCloud``) advected on the GPU after every ``every``-th sim step of ``step()`` while it is
    active.  Tracers that reach the inflow or an outflow face return to their seeds; walls and jets stop them.  ``reset()`` reseeds
    every env's tracers, ``reset_envs(envs)`` those of the chosen envs; ``get_state()`` carries the cloud under ``"mesh_tracers"`` while
    one is active; ``close()`` drops cloud and mesh tables: the cloud is one entry of the env's hook list (``envs/step_hooks.py``).
    Without an active cloud the step path launches nothing."""
    _point_mesh = None

    def _require_multi_block(self, entry: str):
        from ..simulation.mb_tracers import MbPointMesh
        from ..simulation.multiblock import MultiBlockDomain

        if getattr(self, "_domain", None) is None:
            raise RuntimeError(f"{entry}: reset() the env first (the domain does not exist yet)")
        if not isinstance(self._domain, MultiBlockDomain):
            raise NotImplementedError(f"{entry} needs a multi-block domain (cylinder, airfoil envs); single-block envs have probe and "
                                      "start_tracers")
        if self._point_mesh is None or self._point_mesh.domain is not self._domain:
            self._point_mesh = MbPointMesh(self._domain)
        return self._point_mesh

    def _require_single_block(self, entry: str) -> None:
        try:
            super()._require_single_block(entry)
        except NotImplementedError as e:
            raise NotImplementedError(f"{e}; multi-block envs have locate_probes, start_mesh_tracers and stop_mesh_tracers") from None

    @property
    def mesh_tracers(self):
        """The active ``MeshTracerCloud``, or None."""
        return self._hook("mesh_tracers")

    def locate_probes(self, points, strict: bool = True):
        """``MeshProbes`` at the physical positions ``points`` (``[P, d]`` for every env, or ``[B, P, d]``): located once here;
        ``.sample(fields)`` is one launch per call.  ``strict``: a point outside the fluid is a ``ValueError``."""
        from ..simulation.mb_tracers import MeshProbes

        return MeshProbes(self._require_multi_block("locate_probes"), points, strict=strict)

    def _mesh_respawn_faces(self) -> list:
        """The ``(block, face)`` pairs at which a tracer returns to its seed: the inflow face of the left block and the outflow faces."""
        mesh = self._mesh
        return [(0, "-x")] + list(getattr(mesh, "outflows", None) or [mesh.outflow])

    def _mesh_respawn_slots(self) -> np.ndarray:
        from ..simulation.multiblock import face_index

        dom = self._domain
        mask = np.zeros(max(dom.n_boundary_faces, 1), np.uint8)
        for b, face in self._mesh_respawn_faces():
            blk, f = dom.blocks[b], face_index(face)
            s0 = blk.boundary_slot0[f]
            if s0 < 0:
                raise ValueError(f"face {face} of block {blk.name} is not a FIXED boundary")
            mask[s0:s0 + blk.face_cells(f)] = 1
        return mask[:dom.n_boundary_faces]

    def start_mesh_tracers(self, n: int, seed: Optional[int] = None, positions=None, substeps: int = 4, every: int = 1):
        """Start a fresh cloud of ``n`` tracers per env (``MeshTracerCloud``: ``seed`` or ``positions``); after every ``every``-th sim step
        of ``step()`` it is advanced by ``every`` sim time steps in the velocity field of that moment.  Every ``single_step()`` of
        ``MultiBlockSimulation`` advances the flow by exactly ``time_step`` (the adaptive CFL only splits that interval into sub-steps
        inside the call), so the ``every`` sim steps since the last advance lasted ``every * time_step`` whatever their sub-steps
        were: tracer time equals sim time."""
        from ..simulation.mb_tracers import MeshTracerCloud

        mesh = self._require_multi_block("start_mesh_tracers")
        cloud = MeshTracerCloud(mesh, n, seed=seed, positions=positions, substeps=substeps, respawn_slots=self._mesh_respawn_slots().astype(bool))
        return self._start_hook("mesh_tracers", cloud, every,
                                lambda: cloud.advect(self._step_hooks["mesh_tracers"].every * float(self._sim.time_step)),
                                reseed=cloud.reseed, state_key="mesh_tracers")

    def stop_mesh_tracers(self):
        """Stop advecting and hand out the cloud."""
        self._require_multi_block("stop_mesh_tracers")
        return self._stop_hook("mesh_tracers", "stop_mesh_tracers: no tracers are active")
