"""Per-row counter-based Gaussian noise for ``SensorNoise`` / ``ActionNoise`` (``csrc/fg_obsnoise.hip``).

The reference draws ``torch.randn(tensor.shape, generator=g)`` over the whole tensor: in a batch the noise of env 7 would depend on the
batch size and on every other env's history, the generator's position is not part of ``get_state()``, and ``reset_envs`` could not
keep the streams of the untouched envs in place.  Here the noise is a pure function of (seed, row, that row's episode number, that
row's step number, tensor tag, element), computed by ``fg_obs_noise_add`` from Philox4x32-10 -- one launch per observation dict.  A
*row* is one space-shaped item: rows are numbered in C order of the leading axes (env axis, agent axis) of a tensor, plus
``first_row``.  All that is remembered is a device tensor ``[rows, 2]`` of (episode, step) words, updated with stream-ordered torch ops
(no host read, no synchronisation) and carried by ``get_state()`` / ``set_state()``:

* ``reset()`` increments every row's episode and zeroes its step;
* ``reset_envs(envs)`` does so for the rows of the chosen envs only: the others keep their stream;
* ``step()`` increments every row's step (the k-th step of an episode has step word k, its reset observation step word 0).

The words are unsigned 32-bit; the tensor is held as ``int32`` with the same bits, because torch has no ``uint32`` arithmetic.
"""
from __future__ import annotations

import ctypes
from typing import Dict, List, Optional, Sequence

import torch

from .. import _lib as L
from .fluid_wrapper import FluidWrapper
from .util import leading_dims, pop_state_entry, push_state_entry

MAX_SEGMENTS = 8            # segments of one fg_obs_noise_add launch (csrc/fg_obsnoise.hip)
ACTION_TAG = 128            # the tag of the action tensor; observation keys take their index in the sorted key list (< 128)
_DTYPES = {torch.float32: 0, torch.float64: 1}


def noise_add(tensors: Sequence[torch.Tensor], tags: Sequence[int], sigma: float, seed: int, counters: torch.Tensor,
              row_ids: Optional[torch.Tensor] = None) -> List[torch.Tensor]:
    """``t + sigma z`` for every tensor of ``tensors`` as new tensors (the inputs are never written): each is ``rows`` contiguous rows,
    ``rows = counters.shape[0]``, tensor ``j`` with tag ``tags[j]``.  One ``fg_obs_noise_add`` launch per 8 tensors, asynchronous on the
    current stream; there is no other path."""
    rows = int(counters.shape[0])
    out: List[torch.Tensor] = []
    segs = []
    for t, tag in zip(tensors, tags):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise L.NativeLibraryError("the noise wrappers need tensors on the GPU; fluidgym_amd has no CPU path")
        if t.dtype not in _DTYPES or t.dtype != tensors[0].dtype:
            raise TypeError(f"the noise wrappers take float32 or float64 tensors of one dtype, got {t.dtype}")
        if t.numel() == 0 or t.numel() % rows:
            raise ValueError(f"a tensor of shape {tuple(t.shape)} does not hold {rows} rows")
        src = t.detach().contiguous()
        dst = torch.empty_like(src)
        out.append(dst)
        n = src.numel() // rows
        segs.append((L.FgNoiseSegment(src.data_ptr(), dst.data_ptr(), n, n, n, int(tag), float(sigma)), src))
    if not segs:
        return out
    lib = L.load()
    dev = tensors[0].device
    if counters.device != dev or counters.dtype != torch.int32 or not counters.is_contiguous():
        raise ValueError("counters: a contiguous int32 tensor [rows, 2] on the tensors' device")
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    ids = ctypes.c_void_p(row_ids.data_ptr()) if row_ids is not None else None
    for first in range(0, len(segs), MAX_SEGMENTS):
        chunk = segs[first: first + MAX_SEGMENTS]
        arr = (L.FgNoiseSegment * len(chunk))(*[s for s, _ in chunk])
        L.check(lib.fg_obs_noise_add(arr, len(chunk), rows, _DTYPES[tensors[0].dtype], int(seed) & 0xFFFFFFFFFFFFFFFF,
                                     ctypes.c_void_p(counters.data_ptr()), ids, stream))
    return out


class CounterNoiseWrapper(FluidWrapper):
    """What ``SensorNoise`` and ``ActionNoise`` share: sigma, seed, ``first_row`` and the per-row (episode, step) words."""

    _state_key = "noise_counters"

    def __init__(self, env, sigma: float, seed: int, *, first_row: int = 0) -> None:
        super().__init__(env)
        if int(first_row) < 0:
            raise ValueError("first_row must not be negative")
        self._sigma = float(sigma)
        self._noise_seed = int(seed)
        self._first_row = int(first_row)
        self._counters: Optional[torch.Tensor] = None       # int32 [rows, 2]: the bits of the uint32 (episode, step) words
        self._row_ids: Optional[torch.Tensor] = None

    # ---- rows and their counters
    @staticmethod
    def _rows_of(tensor: torch.Tensor, space) -> int:
        rows = 1
        for s in tensor.shape[: leading_dims(tensor, space)]:
            rows *= int(s)
        return rows

    def _obs_rows(self, obs) -> int:
        space = self._env.observation_space
        if isinstance(obs, dict):
            key = sorted(obs)[0]
            return self._rows_of(obs[key], space.spaces[key])
        return self._rows_of(obs, space)

    def _device_of(self, obs) -> torch.device:
        t = obs[sorted(obs)[0]] if isinstance(obs, dict) else obs
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise L.NativeLibraryError(f"{type(self).__name__} needs tensors on the GPU; fluidgym_amd has no CPU path")
        return t.device

    def _ensure_counters(self, rows: int, device: torch.device) -> torch.Tensor:
        if self._counters is None:
            self._counters = torch.zeros((rows, 2), dtype=torch.int32, device=device)
        elif self._counters.shape[0] != rows:
            raise ValueError(f"{type(self).__name__}: {rows} rows where the counters hold {self._counters.shape[0]}")
        if self._first_row and self._row_ids is None:
            self._row_ids = torch.arange(self._first_row, self._first_row + rows, dtype=torch.int32, device=device)
        return self._counters

    def _begin_episode(self, obs) -> None:
        c = self._ensure_counters(self._obs_rows(obs), self._device_of(obs))
        c[:, 0] += 1
        c[:, 1] = 0

    def _begin_episode_envs(self, envs, obs) -> None:
        from ..simulation.state_bank import normalize_envs

        c = self._ensure_counters(self._obs_rows(obs), self._device_of(obs))
        num_envs = int(self._env.num_envs)
        chosen = torch.as_tensor(normalize_envs(envs, num_envs), dtype=torch.int64, device=c.device)
        per_env = c.view(num_envs, c.shape[0] // num_envs, 2)
        per_env[chosen, :, 0] += 1
        per_env[chosen, :, 1] = 0

    def _noisy(self, tensors: Sequence[torch.Tensor], tags: Sequence[int]) -> List[torch.Tensor]:
        return noise_add(tensors, tags, self._sigma, self._noise_seed, self._counters, self._row_ids)

    @property
    def noise_counters(self) -> Optional[torch.Tensor]:
        """The (episode, step) words ``[rows, 2]`` (None before the first reset), as the ``int32`` tensor that holds their bits."""
        return self._counters

    # ---- state: the inner state with this wrapper's counters under a key of its own
    def get_state(self):
        return push_state_entry(self._env.get_state(), self._state_key, None if self._counters is None else self._counters.clone(),
                                type(self).__name__)

    def set_state(self, state) -> None:
        rest, counters = pop_state_entry(state, self._state_key, type(self).__name__)
        self._env.set_state(rest)
        self._counters = None if counters is None else counters.clone()
        self._row_ids = None
        if self._counters is not None:
            self._ensure_counters(int(self._counters.shape[0]), self._counters.device)


class SensorNoise(CounterNoiseWrapper):
    """Gaussian noise with standard deviation ``sigma`` on every tensor of the observation (reference
    ``fluidgym/wrappers/sensor_noise.py``), from the per-row counter-based stream of this module.  Every key of the dict goes through
    one kernel launch (tag: the key's index in the sorted key list); the env's own tensors are never written.

    Parameters
    ----------
    env:
        The environment to wrap.
    sigma: float
        The standard deviation of the noise.
    seed: int
        The seed of the noise stream (its 64 bits are the Philox key).
    first_row: int
        The number of this env's first row in a larger population (for shards wrapped separately).
    """

    _state_key = "sensor_noise_counters"

    def _add_noise(self, obs):
        if not isinstance(obs, dict):
            return self._noisy([obs], [0])[0]
        keys = sorted(obs)
        if len(keys) > ACTION_TAG:
            raise ValueError(f"SensorNoise supports at most {ACTION_TAG} observation keys")
        noisy = dict(zip(keys, self._noisy([obs[k] for k in keys], range(len(keys)))))
        return {k: noisy[k] for k in obs}

    def reset(self, seed: Optional[int] = None, randomize: Optional[bool] = None):
        obs, info = self._env.reset(seed=seed, randomize=randomize)
        self._begin_episode(obs)
        return self._add_noise(obs), info

    def reset_envs(self, envs, randomize: Optional[bool] = None):
        obs = self._env.reset_envs(envs, randomize=randomize)
        self._begin_episode_envs(envs, obs)
        return self._add_noise(obs)

    def step(self, action: torch.Tensor):
        if self._counters is None:
            raise RuntimeError("SensorNoise: call reset() through the wrapper before step()")
        obs, reward, terminated, truncated, info = self._env.step(action)
        self._counters[:, 1] += 1
        return self._add_noise(obs), reward, terminated, truncated, info


class ActionNoise(CounterNoiseWrapper):
    """Gaussian noise with standard deviation ``sigma`` on the action handed to the wrapped env (reference
    ``fluidgym/wrappers/action_noise.py``), from the per-row counter-based stream of this module: tag 128, the counters of the step
    being taken.  No clipping, as in the reference.

    Parameters
    ----------
    env:
        The environment to wrap.
    sigma: float
        The standard deviation of the noise.
    seed: int
        The seed of the noise stream (its 64 bits are the Philox key).
    first_row: int
        The number of this env's first row in a larger population (for shards wrapped separately).
    """

    _state_key = "action_noise_counters"

    def reset(self, seed: Optional[int] = None, randomize: Optional[bool] = None):
        obs, info = self._env.reset(seed=seed, randomize=randomize)
        self._begin_episode(obs)
        return obs, info

    def reset_envs(self, envs, randomize: Optional[bool] = None):
        obs = self._env.reset_envs(envs, randomize=randomize)
        self._begin_episode_envs(envs, obs)
        return obs

    def step(self, action: torch.Tensor):
        if self._counters is None:
            raise RuntimeError("ActionNoise: call reset() through the wrapper before step()")
        if not isinstance(action, torch.Tensor) or not action.is_cuda:
            raise L.NativeLibraryError("ActionNoise needs the action on the GPU; fluidgym_amd has no CPU path")
        rows = self._rows_of(action, self._env.action_space)
        if rows != self._counters.shape[0]:
            raise ValueError(f"ActionNoise: an action of {rows} rows where the counters hold {self._counters.shape[0]}")
        self._counters[:, 1] += 1
        try:
            noisy = self._noisy([action], [ACTION_TAG])[0]
            return self._env.step(noisy)
        except Exception:
            self._counters[:, 1] -= 1       # the step was not taken
            raise
