"""``start_signal_spectra`` / ``stop_signal_spectra`` of every env family: online Welch power and cross spectra
(``simulation/signal_spectra.SignalSpectra``) of a few scalar signals per env -- the drag and lift coefficients of the cylinder and
airfoil envs, field values at probe points, whatever a callable returns -- sampled on the GPU after every ``every``-th sim step of
``step()``, without a host round trip.

The recorder is no ``StepHook`` (``HOOK_ORDER`` is closed): the mixin extends ``_after_sim_step``, ``_reseed_hooks`` and
``_load_hooks_state`` of ``StepHooksMixin`` and runs after the hooks.  ``reset()`` and ``set_state()`` drop every env's open segment,
``reset_envs(envs)`` / ``reset_mesh_envs(envs)`` those of the chosen envs: no segment straddles an episode boundary or a restored
state, while the sums survive until ``stop_signal_spectra()``.  The record does not travel in ``get_state()``, as those of the other
statistics recorders; ``FluidEnv.close()`` drops it.  Without an active recorder the step, reset and state paths do nothing for it.

Cost of a sample: one launch of ``fg_signal_spectra``, one launch per probe set, whatever the callables launch, and for the built-in
``"drag"`` / ``"lift"`` one launch of the wall forces of their own (``_step_impl`` takes its own forces after the hooks)."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, List, Optional

import torch

from ..simulation.signal_spectra import MAX_SOURCES, SignalSpectra, check_extents


@dataclass
class _Active:
    recorder: SignalSpectra
    every: int
    sources: List[Callable[[], torch.Tensor]]
    prepare: Optional[Callable[[], None]] = None      # what the built-in sources share, once per sample
    tick: int = 0


class SignalSpectraMixin:
    _signal_spectra_active: Optional[_Active] = None

    @property
    def signal_spectra(self) -> Optional[SignalSpectra]:
        """The live recorder, or None."""
        active = self._signal_spectra_active
        return None if active is None else active.recorder

    def _signal_sample_time(self) -> float:
        """The time one sim step advances the flow by: ``_sim_step_time()`` on single-block envs; every ``single_step()`` of a
        multi-block simulation advances by exactly ``time_step``."""
        from ..simulation.domain import Domain

        return self._sim_step_time() if isinstance(self._domain, Domain) else float(self._sim.time_step)

    def _builtin_signals(self) -> dict:
        """name -> index into ``(drag, lift)``: the normalised coefficients of ``_get_drag_and_lift``, on the envs that have them."""
        return {"drag": 0, "lift": 1} if hasattr(self, "_get_drag_and_lift") else {}

    def start_signal_spectra(self, signals=(), probes=None, probe_fields=None, segment: int = 256, noverlap: Optional[int] = None,
                             window="hann", detrend: str = "constant", pairs=(), every: int = 1) -> SignalSpectra:
        """Start a fresh recorder (in place of an earlier one) and return it.

        ``signals``: names and / or a mapping ``name -> callable(env)`` that returns ``[B]`` or ``[B, n]`` on the env's device
        (columns named ``name[i]``); a sequence may mix names and ``(name, callable)`` pairs.  Built-in names on the cylinder and
        airfoil envs: ``"drag"`` and ``"lift"``, the coefficients of ``_get_drag_and_lift``, summed over the span in 3-D.  Every
        callable is evaluated once here, to learn its width.
        ``probes``: physical points ``[P, d]`` or ``[B, P, d]``, uploaded (multi-block envs: located) once and sampled in one launch
        per sample; ``probe_fields`` default to the env's ``u, v(, w), p(, T)``; the signals are named ``"{field}@{p}"``.
        ``segment``, ``noverlap``, ``window``, ``detrend``, ``pairs``: the spec of ``SignalSpectraRecord``; the sample interval is
        ``every`` times the sim-step time.  At most 8 sources (callables, built-ins together, the probe set) and 64 signals."""
        if getattr(self, "_domain", None) is None:
            raise RuntimeError("start_signal_spectra: reset() the env first (the domain does not exist yet)")
        if int(every) < 1:
            raise ValueError(f"every must be at least 1, got {every}")
        check_extents(segment, self._dtype, "start_signal_spectra")
        items = list(signals.items()) if isinstance(signals, dict) else [s if isinstance(s, str) else tuple(s) for s in signals]
        builtin, names, sources, prepare = self._builtin_signals(), [], [], None
        forces = {}
        for item in items:
            if isinstance(item, str) or item[1] is None:
                name = item if isinstance(item, str) else item[0]
                if name not in builtin:
                    raise ValueError(f"start_signal_spectra: {type(self).__name__} has no built-in signal {name!r} "
                                     f"(built in: {tuple(builtin) or 'none'}); give a callable for it")
                if prepare is None:
                    def prepare(forces=forces):
                        cd, cl = self._get_drag_and_lift()
                        forces[0], forces[1] = (cd.sum(-1), cl.sum(-1)) if cd.dim() == 2 else (cd, cl)
                sources.append(lambda k=builtin[name]: forces[k])
                names.append((name, None))
            else:
                name, fn = item
                sources.append(lambda fn=fn: fn(self))
                names.append((str(name), fn))
        if probes is not None:
            sources.append(self._probe_signal_source(probes, probe_fields))
            names.append(("@", probe_fields))
        if not 1 <= len(sources) <= MAX_SOURCES:
            raise ValueError(f"start_signal_spectra: 1..{MAX_SOURCES} sources (callables, built-in names, the probe set), got "
                             f"{len(sources)}; let one callable return several columns [B, n]")
        # one evaluation to learn the widths, hence the names
        if prepare is not None:
            prepare()
        flat = []
        for (name, tag), src in zip(names, sources):
            first = src()
            if not isinstance(first, torch.Tensor) or first.dim() not in (1, 2) or first.shape[0] != self._num_envs:
                raise ValueError(f"start_signal_spectra: the source of {name!r} must return a tensor [B] or [B, n] with "
                                 f"B = {self._num_envs}, got {getattr(first, 'shape', type(first))}")
            if name == "@":
                fields = self._probe_field_names(tag)
                flat += [f"{f}@{p}" for p in range(first.shape[1] // len(fields)) for f in fields]
            else:
                flat += [name] if first.dim() == 1 else [f"{name}[{i}]" for i in range(first.shape[1])]
        recorder = self._make_signal_recorder(flat, segment, noverlap, window, detrend, pairs, int(every) * self._signal_sample_time())
        self._signal_spectra_active = _Active(recorder, int(every), sources, prepare)
        return recorder

    def _make_signal_recorder(self, *spec) -> SignalSpectra:
        return SignalSpectra(*spec)

    def _probe_field_names(self, probe_fields) -> tuple:
        if probe_fields is not None:
            return tuple(probe_fields)
        from ..simulation.domain import Domain
        from ..simulation.tracers import default_fields

        if isinstance(self._domain, Domain):
            return tuple(default_fields(self._domain))
        return ("u", "v") + (("w",) if self._ndims == 3 else ()) + ("p",)

    def _probe_signal_source(self, probes, probe_fields) -> Callable[[], torch.Tensor]:
        """The probe set as one source ``[B, P * K]`` (point-major): one launch per sample."""
        from ..simulation.domain import Domain

        fields = None if probe_fields is None else tuple(probe_fields)
        if isinstance(self._domain, Domain):
            pts = torch.as_tensor(probes, dtype=torch.float64).to(self._domain.device, self._domain.dtype).contiguous()
            self.probe(pts, fields)                                   # refuses bad points here and not at the first sample
            return lambda: self.probe(pts, fields).flatten(1)
        located = self.locate_probes(probes)
        return lambda: located.sample(fields).flatten(1)

    def stop_signal_spectra(self) -> SignalSpectra:
        """Stop sampling and hand out the recorder (``.record()`` is its host copy)."""
        active = self._signal_spectra_active
        if active is None:
            raise RuntimeError("stop_signal_spectra: no signal spectra are being recorded")
        self._signal_spectra_active = None
        return active.recorder

    # ---- the wiring: after the hooks of StepHooksMixin
    def _after_sim_step(self) -> None:
        super()._after_sim_step()
        active = self._signal_spectra_active
        if active is None:
            return
        active.tick += 1
        if active.tick % active.every == 0:
            if active.prepare is not None:
                active.prepare()
            active.recorder.update(*[src() for src in active.sources])

    def _reseed_hooks(self, envs=None) -> None:
        super()._reseed_hooks(envs)
        active = self._signal_spectra_active
        if active is not None:
            active.recorder.restart(envs)
            if envs is None:
                active.tick = 0

    def _load_hooks_state(self, state: dict) -> None:
        super()._load_hooks_state(state)
        active = self._signal_spectra_active
        if active is not None:                                        # a restored state continues no open segment
            active.recorder.restart(None)
            active.tick = 0
