"""``FluidWrapper``: the base class of the env wrappers (reference ``fluidgym/wrappers/fluid_wrapper.py``).

Same members, parameter names and defaults as the reference's base class; every member of the ``FluidEnvLike`` protocol is forwarded
to the wrapped env explicitly, and anything else -- ``num_envs``, ``reset_envs``, ``render_frames``, ``start_*`` / ``stop_*`` and the
other additions of this package -- reaches it through ``__getattr__``.  It wraps a ``FluidEnv`` (un-batched or batched), a
``ParallelFluidEnv`` or another wrapper.
"""
from __future__ import annotations

from pathlib import Path
from typing import Any, Optional

import torch

from ..types import EnvMode


class FluidWrapper:
    """A wrapper that changes nothing: subclasses override what they change.

    Parameters
    ----------
    env:
        The environment (or wrapper) to wrap.
    """

    def __init__(self, env) -> None:
        self._env = env

    def __getattr__(self, name: str) -> Any:
        # only reached when the normal lookup on the wrapper fails
        if name == "_env":      # (not set yet: a constructor that raised must not recurse through this hook)
            raise AttributeError(name)
        return getattr(self._env, name)

    @property
    def unwrapped(self):
        """The innermost environment, below every wrapper."""
        env = self._env
        while isinstance(env, FluidWrapper):
            env = env._env
        return env

    # ---- the members of FluidEnvLike, forwarded
    @property
    def use_marl(self) -> bool:
        return self._env.use_marl

    @property
    def n_agents(self) -> int:
        return self._env.n_agents

    @property
    def episode_length(self) -> int:
        return self._env.episode_length

    @property
    def metrics(self):
        return self._env.metrics

    @property
    def cuda_device(self) -> torch.device:
        return self._env.cuda_device

    @property
    def differentiable(self) -> bool:
        return self._env.differentiable

    @property
    def action_space(self):
        return self._env.action_space

    @property
    def observation_space(self):
        return self._env.observation_space

    def train(self) -> None:
        self._env.train()

    def val(self) -> None:
        self._env.val()

    def test(self) -> None:
        self._env.test()

    def sample_action(self) -> torch.Tensor:
        return self._env.sample_action()

    def step(self, action: torch.Tensor):
        return self._env.step(action)

    def seed(self, seed: int) -> None:
        self._env.seed(seed)

    def reset(self, seed: Optional[int] = None, randomize: Optional[bool] = None):
        return self._env.reset(seed=seed, randomize=randomize)

    def render(self, save: bool = False, render_3d: bool = False, filename: Optional[str] = None, output_path: Optional[Path] = None):
        return self._env.render(save=save, render_3d=render_3d, filename=filename, output_path=output_path)

    def save_gif(self, filename: str, output_path: Optional[Path] = None) -> None:
        self._env.save_gif(filename=filename, output_path=output_path)

    def load_initial_domain(self, idx: int, mode: Optional[EnvMode] = None) -> None:
        self._env.load_initial_domain(idx=idx, mode=mode)

    def get_uncontrolled_episode_metrics(self):
        return self._env.get_uncontrolled_episode_metrics()

    def detach(self) -> None:
        self._env.detach()

    def get_state(self):
        return self._env.get_state()

    def set_state(self, state) -> None:
        return self._env.set_state(state)
