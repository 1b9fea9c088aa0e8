"""The consumers that run after a sim step inside ``step()`` while they are switched on: the recorders of ``envs/flow_statistics.py``
and the tracer clouds of ``envs/tracers.py``.  An env keeps its active ones as ``StepHook`` records in one mapping, ``_step_hooks``,
empty by default, and its sim-step loop calls ``_after_sim_step()`` once per sim step: every hook counts the step and runs at every
``every``-th one.  The hooks run in the order of ``HOOK_ORDER`` whatever order they were started in, so a step issues the same
launches in the same order.  ``reset``, ``reset_envs``, ``get_state``, ``set_state`` and ``close`` of ``FluidEnv`` go through the same
mapping: a hook with ``reseed`` returns to its seeds there, one with a ``state_key`` travels in the env's state under that key.

The frame recorder is no hook: it samples per env step, after the counters, and owns its tick."""
from __future__ import annotations

from dataclasses import dataclass
from types import MappingProxyType
from typing import Any, Callable, Mapping, Optional

HOOK_ORDER = ("flow_stats", "flow_spectra", "flow_budgets", "flow_timecorr", "flow_hist", "field_stats", "tracers", "mesh_tracers")
# state_key -> (what it holds, the entry that starts one): the keys a state can carry, for set_state's refusal
STATE_KEYS = {"tracers": ("tracer cloud", "start_tracers"), "mesh_tracers": ("mesh tracer cloud", "start_mesh_tracers")}


@dataclass
class StepHook:
    name: str                   # one of HOOK_ORDER
    target: Any                 # the recorder or cloud that start_* made and stop_* hands out
    every: int
    run: Callable[[], None]     # the work of one due sim step; it does not count
    tick: int = 0
    reseed: Optional[Callable[[Any], None]] = None      # reseed(None): every env, reseed(envs): the chosen ones
    state_key: Optional[str] = None                     # the target has state_dict() / load_state_dict()


class StepHooksMixin:
    _step_hooks: Mapping[str, StepHook] = MappingProxyType({})      # in the order of HOOK_ORDER; replaced, never changed in place

    def _start_hook(self, name: str, target, every: int, run, reseed=None, state_key: Optional[str] = None):
        """Make ``target`` the active consumer ``name`` (in place of an earlier one) with its tick at zero; returns ``target``."""
        if name not in HOOK_ORDER:
            raise KeyError(f"{name!r} has no place in HOOK_ORDER")
        if int(every) < 1:
            raise ValueError(f"every must be at least 1, got {every}")
        hooks = {**self._step_hooks, name: StepHook(name, target, int(every), run, reseed=reseed, state_key=state_key)}
        self._step_hooks = {n: hooks[n] for n in HOOK_ORDER if n in hooks}
        return target

    def _stop_hook(self, name: str, refusal: str):
        """Take the consumer ``name`` off the list and hand out its target; ``RuntimeError(refusal)`` when it is not active (the
        caller's "stop_x: no x are being recorded")."""
        if name not in self._step_hooks:
            raise RuntimeError(refusal)
        hooks = dict(self._step_hooks)
        target = hooks.pop(name).target
        self._step_hooks = hooks
        return target

    def _hook(self, name: str):
        """The target of the active consumer ``name``, or None."""
        hook = self._step_hooks.get(name)
        return None if hook is None else hook.target

    def _after_sim_step(self) -> None:
        for hook in self._step_hooks.values():
            hook.tick += 1
            if hook.tick % hook.every == 0:
                hook.run()

    def _reseed_hooks(self, envs=None) -> None:
        """``reset()`` (``envs`` None: every env returns to its seeds and the ticks to zero) and ``reset_envs(envs)`` (the chosen envs;
        the ticks stay) for the hooks that have seeds."""
        for hook in self._step_hooks.values():
            if hook.reseed is not None:
                hook.reseed(envs)
                if envs is None:
                    hook.tick = 0

    def _hooks_state(self) -> dict:
        """What ``get_state()`` carries of the hooks: ``state_key -> {"cloud", "every", "tick"}``."""
        return {h.state_key: {"cloud": h.target.state_dict(), "every": h.every, "tick": h.tick}
                for h in self._step_hooks.values() if h.state_key is not None}

    def _load_hooks_state(self, state: dict) -> None:
        """``set_state()``: every ``STATE_KEYS`` entry of ``state`` goes back into the active hook of that key; ``RuntimeError``
        without one (a cloud's size is not part of the state)."""
        active = {h.state_key: h for h in self._step_hooks.values()}
        for key, (what, entry) in STATE_KEYS.items():
            if key not in state:
                continue
            if key not in active:
                raise RuntimeError(f"set_state: the state holds a {what} but none is active; call {entry}() with its size first")
            hook, saved = active[key], state[key]
            hook.target.load_state_dict(saved["cloud"])
            hook.every, hook.tick = int(saved["every"]), int(saved["tick"])
