"""``start_flow_statistics`` / ``stop_flow_statistics`` of the wall-bounded single-block envs (TCF, RBC): one sample of the
plane-averaged statistics (``simulation/plane_stats.PlaneMoments``) after every ``every``-th sim step, on the GPU, while active.
The reference records them from its run scripts with ``VelocityStats.record_vel_stats`` (``TCF_tools.py:1480-1507``).
``start_flow_spectra`` / ``stop_flow_spectra`` do the same, independently, for the wavenumber spectra of chosen wall-parallel
planes (``simulation/plane_spectra.PlaneSpectra``; the reference's ``PSD_planes``, ``TCF_tools.py:445-459, 1491-1500``), and
``start_flow_budgets`` / ``stop_flow_budgets`` for the Reynolds-stress budgets of 3-D channels
(``simulation/plane_budgets.PlaneBudgets``; the reference's ``TurbulentEnergyBudgetsOnlineParallel_Torch``,
``TCF_tools.py:438-443, 1512-1516``), and ``start_flow_time_correlation`` / ``stop_flow_time_correlation`` for the temporal two-point
correlations of the planes (``simulation/plane_timecorr.PlaneTimeCorrelation``; the reference's
``TemporalTwoPointCorrelation_Online_torch``, ``TCF_tools.py:431-436, 1508-1511``), and ``start_flow_histograms`` /
``stop_flow_histograms`` for the PDFs and joint PDFs of chosen rows (``simulation/plane_hist.PlaneHistograms``; the reference records
no distributions).

The multi-block envs (cylinder, airfoil) have no homogeneous plane; ``FieldStatisticsMixin`` gives them ``start_field_statistics`` /
``stop_field_statistics``: the time-averaged fields per cell, in 3-D averaged over the span as well
(``simulation/cell_moments.CellMoments``; the reference's ``WelfordOnlineParallel_Torch`` / ``CovarianceOnlineParallel_Torch`` per
block).

Every ``start_*`` checks its own arguments, makes the recorder and hands it to ``_start_hook`` (``envs/step_hooks.py``) with the one
line that takes a sample; every ``stop_*`` is one ``_stop_hook``.  Counting the sim steps, the order among the recorders and an env
with nothing switched on are the hook list's business."""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np

from ..simulation.cell_moments import CellMoments
from ..simulation.plane_budgets import PlaneBudgets
from ..simulation.plane_hist import CHANNEL_ORDER, PlaneHistograms
from ..simulation.plane_spectra import PlaneSpectra, check_extents
from ..simulation.plane_stats import CHANNEL_SETS, PlaneMoments
from ..simulation.plane_timecorr import PlaneTimeCorrelation


def _check_start(env, entry: str, single_block: Optional[str] = None, needs_3d: bool = False) -> None:
    """The checks every ``start_*`` begins with: reset() done, (``single_block``: what needs one) a single-block domain, (``needs_3d``)
    a 3-D one.  (``every`` is checked by ``_start_hook``.)"""
    if getattr(env, "_domain", None) is None:
        raise RuntimeError(f"{entry}: reset() the env first (the domain does not exist yet)")
    if single_block is not None and env._flow_blocks() != 1:
        raise NotImplementedError(f"{single_block} need a single-block domain")
    if needs_3d and env._ndims != 3:
        raise NotImplementedError(f"{single_block} need a 3-D domain")


class FlowStatisticsMixin:
    _flow_stats_scalar: bool = False                # whether the passive scalar is recorded as channel T

    def _flow_blocks(self) -> int:
        count = getattr(self._domain, "getNumBlocks", None)
        return count() if count is not None else len(self._domain.blocks)       # (the multi-block domain keeps a list)

    def _flow_channels(self):
        return ("u", "v") + (("w",) if self._ndims == 3 else ()) + ("p",) + (("T",) if self._flow_stats_scalar else ())

    def _flow_fields(self, channels) -> tuple:
        """``(velocity, pressure, scalar)`` of the block as bound now, None for a field that is no channel of ``channels``."""
        blk = self._domain.getBlock(0)
        return blk.velocity, blk.pressure if "p" in channels else None, blk.passiveScalar if "T" in channels else None

    def start_flow_statistics(self, order: int = 2, every: int = 1) -> None:
        """Start a fresh record of moments up to ``order``; a sample is taken after every ``every``-th sim step of ``step()``."""
        _check_start(self, "start_flow_statistics", "flow statistics")
        stats = PlaneMoments(self._flow_channels(), order)
        self._start_hook("flow_stats", stats, every, lambda: stats.update(*self._flow_fields(stats.channels)))

    def stop_flow_statistics(self) -> PlaneMoments:
        """Stop recording and hand out the record (on the GPU; its accessors, ``pooled()`` and ``save`` read it back)."""
        return self._stop_hook("flow_stats", "stop_flow_statistics: no statistics are being recorded")

    def start_flow_spectra(self, planes: Sequence[int], every: int = 1, symmetric: bool = True) -> None:
        """Start a fresh record of the wavenumber spectra of the rows ``planes`` (and, ``symmetric``, of their mirror images) of
        the channels of the moments; a sample is taken after every ``every``-th sim step of ``step()``."""
        _check_start(self, "start_flow_spectra", "flow spectra")
        vel = self._domain.getBlock(0).velocity
        nz, ny, nx = ((1,) + tuple(int(s) for s in vel.shape[2:]))[-3:]
        check_extents(nz, nx, vel.element_size(), "start_flow_spectra")
        spectra = PlaneSpectra(self._flow_channels(), planes, symmetric)
        spectra.plane_table(ny)                            # planes outside the grid are refused here, not at the first sample
        self._start_hook("flow_spectra", spectra, every, lambda: spectra.update(*self._flow_fields(spectra.channels)))

    def stop_flow_spectra(self) -> PlaneSpectra:
        """Stop recording and hand out the record (on the GPU; its accessors, ``pooled()`` and ``save`` read it back)."""
        return self._stop_hook("flow_spectra", "stop_flow_spectra: no spectra are being recorded")

    def start_flow_budgets(self, every: int = 1, forcing: Optional[bool] = None) -> None:
        """Start a fresh record of the Reynolds-stress budgets; a sample is taken after every ``every``-th sim step of ``step()``.
        The coordinates are the block's cell centres, periodic x / z faces wrap, ``forcing`` defaults to whether the block has a
        velocity source."""
        _check_start(self, "start_flow_budgets", "flow budgets", needs_3d=True)
        blk = self._domain.getBlock(0)
        if forcing is None:
            forcing = blk.velocitySource is not None
        elif forcing and blk.velocitySource is None:
            raise ValueError("start_flow_budgets: forcing=True needs a block with a velocity source")
        x, y, z = (0.5 * (np.asarray(e, np.float64)[1:] + np.asarray(e, np.float64)[:-1]) for e in blk.edges)
        budgets = PlaneBudgets(x, y, z, forcing=bool(forcing), wrap=(not blk.isFixed("-x"), not blk.isFixed("-z")))

        def sample():
            blk = self._domain.getBlock(0)
            budgets.update(blk.velocity, blk.pressure, blk.velocitySource if budgets.forcing else None)

        self._start_hook("flow_budgets", budgets, every, sample)

    def stop_flow_budgets(self) -> PlaneBudgets:
        """Stop recording and hand out the record (on the GPU; its accessors, ``pooled()`` and ``save`` read it back)."""
        return self._stop_hook("flow_budgets", "stop_flow_budgets: no budgets are being recorded")

    def start_flow_time_correlation(self, lags: int, every: int = 1, stride: Optional[int] = None,
                                    channels: Optional[Sequence[str]] = None) -> None:
        """Start a fresh record of the temporal correlations over ``lags`` samples; a sample is taken after every ``every``-th sim
        step of ``step()``, its time the simulation's host-side clock.  ``stride`` None: one base at the first sample, as the
        reference; ``stride = S``: a new base at every ``S``-th sample.  ``channels`` default to the velocity components; any channel
        set of the moments is taken."""
        _check_start(self, "start_flow_time_correlation", "flow time correlations")
        velocity = ("u", "v") + (("w",) if self._ndims == 3 else ())
        channels = velocity if channels is None else tuple(channels)
        if channels != velocity and (channels not in CHANNEL_SETS or ("w" in channels) != (self._ndims == 3)):
            raise ValueError(f"channels must be {velocity} or one of {CHANNEL_SETS} that fits the {self._ndims}-D domain, got {channels}")
        if "T" in channels and not self._domain.getBlock(0).hasPassiveScalar():
            raise ValueError("start_flow_time_correlation: channel T needs a domain with a passive scalar")
        corr = PlaneTimeCorrelation(channels, lags, stride)
        self._start_hook("flow_timecorr", corr, every,
                         lambda: corr.update(*self._flow_fields(corr.channels), time=self._sim.total_time))

    def stop_flow_time_correlation(self) -> PlaneTimeCorrelation:
        """Stop recording and hand out the record (on the GPU; its accessors, ``pooled()`` and ``save`` read it back)."""
        return self._stop_hook("flow_timecorr", "stop_flow_time_correlation: no time correlations are being recorded")

    def start_flow_histograms(self, ranges=None, bins: int = 128, joint: Sequence = (), joint_bins: int = 32,
                              rows: Optional[Sequence[int]] = None, channels: Optional[Sequence[str]] = None, every: int = 1) -> None:
        """Start a fresh record of the histograms of ``channels`` (default: those of the moments; any of ``u, v, w, p, T`` in that
        order) over the rows ``rows`` (default: all) and of the joint histograms of the channel pairs ``joint``; a sample is taken
        after every ``every``-th sim step of ``step()``.  ``ranges`` maps a channel to ``(lo, hi)`` or to ``[n_rows, 2]``; None takes,
        per listed row and channel, the minimum and maximum over the batch of the current state, widened by half the span on each
        side (by 1 where the span is zero)."""
        _check_start(self, "start_flow_histograms", "flow histograms")
        channels = self._flow_channels() if channels is None else tuple(channels)
        blk = self._domain.getBlock(0)
        if any(c not in CHANNEL_ORDER for c in channels) or ("w" in channels and self._ndims != 3):
            raise ValueError(f"channels must be names from {CHANNEL_ORDER} that fit the {self._ndims}-D domain, got {channels}")
        if "T" in channels and not blk.hasPassiveScalar():
            raise ValueError("start_flow_histograms: channel T needs a domain with a passive scalar")
        ny = int(blk.velocity.shape[-2])
        if rows is not None and (len(rows) < 1 or min(rows) < 0 or max(rows) >= ny):
            raise ValueError(f"rows must lie in [0, {ny}), got {list(rows)}")
        if ranges is None:
            src = {"u": (blk.velocity, 0), "v": (blk.velocity, 1), "w": (blk.velocity, 2), "p": (blk.pressure, 0),
                   "T": (blk.passiveScalar, 0)}
            listed = list(range(ny)) if rows is None else [int(r) for r in rows]
            ranges = {}
            for c in channels:
                t, comp = src[c]
                f = t[:, comp].double().movedim(-2, 0)[listed].flatten(1)               # [R, B * nz * nx]
                lo, hi = f.amin(dim=1).cpu().numpy(), f.amax(dim=1).cpu().numpy()
                pad = np.where(hi > lo, 0.5 * (hi - lo), 1.0)
                ranges[c] = np.stack([lo - pad, hi + pad], axis=1)
        hist = PlaneHistograms(channels, ranges, bins, joint, joint_bins, rows)
        self._start_hook("flow_hist", hist, every, lambda: hist.update(*self._flow_fields(hist.channels)))

    def stop_flow_histograms(self) -> PlaneHistograms:
        """Stop recording and hand out the record (on the GPU; its accessors, ``pooled()`` and ``save`` read it back)."""
        return self._stop_hook("flow_hist", "stop_flow_histograms: no histograms are being recorded")


class FieldStatisticsMixin:
    def start_field_statistics(self, every: int = 1, span_average: bool = True, surface: bool = False) -> None:
        """Start a fresh per-cell record of ``u, v(, w), p``; a sample is taken after every ``every``-th sim step of ``step()`` (the
        fields are read, never written).  ``span_average`` (3-D): one column per ``(block, y, x)``, averaged over the span; off,
        every cell is recorded.  ``surface``: the same hook also records the wall curves ``p, tau_w, fx, fy`` of the env's wall ring
        (``simulation/wall_stats.WallMoments``, one more launch per sample, with the viscosity of the env's drag and lift -- env b's own
        where the batch has one per env); the record ``stop_field_statistics`` hands out carries it as ``.surface`` (None otherwise)."""
        _check_start(self, "start_field_statistics")
        stats = CellMoments.for_domain(self._domain, span_average)
        if not surface:
            self._start_hook("field_stats", stats, every, lambda: stats.update(self._domain.velocity, self._domain.pressure))
            return
        if getattr(self, "_ring", None) is None:
            raise NotImplementedError("start_field_statistics(surface=True) needs an env with a wall ring (cylinder, airfoil envs)")
        wall = stats.surface = self._ring.moments(self._domain.batch, self._domain.dtype, span_average)

        def sample():
            stats.update(self._domain.velocity, self._domain.pressure)
            wall.update(self._domain, self._wall_force_args()[0])

        self._start_hook("field_stats", stats, every, sample)

    def stop_field_statistics(self) -> CellMoments:
        """Stop recording and hand out the record (on the GPU; its accessors, ``pooled()`` and ``save`` read it back)."""
        return self._stop_hook("field_stats", "stop_field_statistics: no field statistics are being recorded")
