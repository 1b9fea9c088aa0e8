"""``start_flow_statistics`` / ``stop_flow_statistics`` of the wall-bounded single-block envs (TCF, RBC): one sample of the
plane-averaged statistics (``simulation/plane_stats.PlaneMoments``) after every ``every``-th sim step, on the GPU, while active.
The reference records them from its run scripts with ``VelocityStats.record_vel_stats`` (``TCF_tools.py:1480-1507``)."""
from __future__ import annotations

from typing import Optional

from ..simulation.plane_stats import PlaneMoments


class FlowStatisticsMixin:
    _flow_stats: Optional[PlaneMoments] = None      # None (the default): the step path does nothing for the statistics
    _flow_stats_every: int = 1
    _flow_stats_tick: int = 0
    _flow_stats_scalar: bool = False                # whether the passive scalar is recorded as channel T

    def start_flow_statistics(self, order: int = 2, every: int = 1) -> None:
        """Start a fresh record of moments up to ``order``; a sample is taken after every ``every``-th sim step of ``step()``."""
        if getattr(self, "_domain", None) is None:
            raise RuntimeError("start_flow_statistics: reset() the env first (the domain does not exist yet)")
        if self._domain.getNumBlocks() != 1:
            raise NotImplementedError("flow statistics need a single-block domain")
        if int(every) < 1:
            raise ValueError(f"every must be at least 1, got {every}")
        channels = ("u", "v") + (("w",) if self._ndims == 3 else ()) + ("p",) + (("T",) if self._flow_stats_scalar else ())
        self._flow_stats = PlaneMoments(channels, order)
        self._flow_stats_every, self._flow_stats_tick = int(every), 0

    def stop_flow_statistics(self) -> PlaneMoments:
        """Stop recording and hand out the record (on the GPU; its accessors, ``pooled()`` and ``save`` read it back)."""
        if self._flow_stats is None:
            raise RuntimeError("stop_flow_statistics: no statistics are being recorded")
        stats, self._flow_stats = self._flow_stats, None
        return stats

    def _record_flow_sample(self) -> None:
        """Called after a sim step while statistics are active."""
        self._flow_stats_tick += 1
        if self._flow_stats_tick % self._flow_stats_every:
            return
        blk = self._domain.getBlock(0)
        self._flow_stats.update(blk.velocity, blk.pressure, blk.passiveScalar if self._flow_stats_scalar else None)
