"""``ObsExtraction``: keep only chosen keys of the observation dict (reference ``fluidgym/wrappers/obs_extraction.py``)."""
from __future__ import annotations

from typing import Dict, List, Optional

import torch

from .. import spaces
from .fluid_wrapper import FluidWrapper


class ObsExtraction(FluidWrapper):
    """Observations and observation space reduced to the keys ``keys``, in that order.

    Parameters
    ----------
    env:
        The environment to wrap; its observation space must be a ``Dict``.
    keys: list[str]
        The keys to keep; not empty, each a key of the observation space.
    """

    def __init__(self, env, keys: List[str]) -> None:
        super().__init__(env)
        if len(keys) == 0:
            raise ValueError("Keys list must be non-empty or None.")
        space = self._env.observation_space
        if not isinstance(space, spaces.Dict):
            raise ValueError("ObsExtraction wrapper only supports Dict observation spaces.")
        for k in keys:
            if k not in space.spaces:
                raise ValueError(f"Key '{k}' not found in observation space.")
        self._keys = list(keys)
        self._observation_space = spaces.Dict({k: space.spaces[k] for k in self._keys})

    @property
    def observation_space(self) -> spaces.Dict:
        return self._observation_space

    def _filter(self, obs: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        return {k: obs[k] for k in self._keys}

    def reset(self, seed: Optional[int] = None, randomize: Optional[bool] = None):
        obs, info = self._env.reset(seed=seed, randomize=randomize)
        return self._filter(obs), info

    def reset_envs(self, envs, randomize: Optional[bool] = None):
        return self._filter(self._env.reset_envs(envs, randomize=randomize))

    def step(self, action: torch.Tensor):
        obs, reward, terminated, truncated, info = self._env.step(action)
        return self._filter(obs), reward, terminated, truncated, info
