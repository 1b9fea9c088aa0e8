"""``FlattenObservation``: the observation dict as one flat tensor (reference ``fluidgym/wrappers/flatten_obs.py``).

The reference flattens from axis 0 (single agent) or 1 (multi agent).  Here a tensor may also carry the env axis of a batch, so the
flattening starts after the leading axes of each tensor -- its ``dim()`` minus the rank of that key's space: ``[B, D]`` for a batch,
``[B, n_agents, D]`` for a multi-agent batch, and what the reference gives for an un-batched env.  Plain torch (``torch.cat``).
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from .. import spaces
from .fluid_wrapper import FluidWrapper
from .util import flatten_dict_space, leading_dims

# the keys the reference flattens, in its order; the others (pressure, ...) are left out of the flat observation, as there
DEFAULT_KEYS = ["temperature", "velocity"]


class FlattenObservation(FluidWrapper):
    """The ``temperature`` and ``velocity`` entries of the observation dict (those the space has), flattened and concatenated.  The
    un-flattened tensors are kept as ``info["original_<key>"]``.

    Parameters
    ----------
    env:
        The environment to wrap; its observation space must be a ``Dict``.
    """

    def __init__(self, env) -> None:
        super().__init__(env)
        space = self._env.observation_space
        if not isinstance(space, spaces.Dict):
            raise ValueError("FlattenObservation wrapper only supports Dict observation spaces.")
        self._keys = [k for k in DEFAULT_KEYS if k in space.spaces]
        self._observation_space = flatten_dict_space(space=space, keys=self._keys)

    @property
    def observation_space(self) -> spaces.Box:
        return self._observation_space

    def _flatten(self, obs: Dict[str, torch.Tensor]) -> torch.Tensor:
        sub = self._env.observation_space.spaces
        parts = []
        for k in self._keys:
            lead = leading_dims(obs[k], sub[k])
            parts.append(obs[k].reshape(tuple(obs[k].shape[:lead]) + (-1,)))
        return torch.cat(parts, dim=-1)

    @staticmethod
    def _keep_originals(obs: Dict[str, torch.Tensor], info) -> None:
        if isinstance(info, dict):
            for k, v in obs.items():
                info["original_" + k] = v
        else:       # ParallelFluidEnv: one info dict per env
            for k, v in obs.items():
                if v.shape[0] == len(info):
                    for i, row in enumerate(v.unbind(0)):
                        info[i]["original_" + k] = row

    def reset(self, seed: Optional[int] = None, randomize: Optional[bool] = None):
        obs, info = self._env.reset(seed=seed, randomize=randomize)
        self._keep_originals(obs, info)
        return self._flatten(obs), info

    def reset_envs(self, envs, randomize: Optional[bool] = None):
        return self._flatten(self._env.reset_envs(envs, randomize=randomize))

    def step(self, action: torch.Tensor):
        obs, reward, terminated, truncated, info = self._env.step(action)
        self._keep_originals(obs, info)
        return self._flatten(obs), reward, terminated, truncated, info
