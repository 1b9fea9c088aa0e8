"""Running normalisation of observations and rewards (``csrc/fg_obsnorm.hip``): what gymnasium calls
``NormalizeObservation`` / ``NormalizeReward`` and SB3 ``VecNormalize``, on the GPU.

A *row* is one space-shaped item, numbered in C order of the leading axes (env axis, agent axis) as in ``noise.py``.  Every statistic
slot keeps the record ``(n, mean, M2)``: ``n`` rows merged so far -- one Python ``int`` shared by all keys, passed to the kernel by
value -- and ``mean`` / ``M2`` as fp64 tensors on the device.  One update with the rows ``R`` (``m = |R|``), all in fp64::

    mean_b = sum_{r in R} x[r] / m;   M2_b = sum_{r in R} (x[r] - mean_b)^2          (two passes)
    delta  = mean_b - mean_a;  n = n_a + m;  mean = mean_a + delta * (m / n);  M2 = M2_a + M2_b + delta^2 * (n_a * m / n)

and the value handed on uses the record after the update, ``y = (x - mean) / sqrt(M2 / n + epsilon)``, clipped to ``[-clip, clip]``
when a clip is given and rounded once to the tensor's dtype.  The record starts EMPTY (``n = 0``), not at gymnasium's
``(count, mean, var) = (1e-4, 0, 1)``: the first batch is normalised by its own moments.  ``pool="element"`` keeps one slot per
element of the space, ``pool="key"`` one scalar slot per key over rows and elements (its count is ``n * D``).  The order of every sum
is a function of ``(m, D, pool)`` alone and is written at the top of ``csrc/fg_obsnorm.hip``, so a run repeats bit for bit; a whole
observation dict is one launch in element mode (two in key mode while updating), the reward one launch.  Nothing synchronises and
nothing reads ``terminated`` / ``truncated``: episodes begin through ``reset()`` and ``reset_envs()`` only.
"""
from __future__ import annotations

import ctypes
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _lib as L
from .. import spaces
from .fluid_wrapper import FluidWrapper
from .util import leading_dims, pop_state_entry, push_state_entry

MAX_SEGMENTS = 8            # segments of one fg_obs_normalize call (csrc/fg_obsnorm.hip)
_DTYPES = {torch.float32: 0, torch.float64: 1}
_SINGLE = "observation"     # the record's key of a single-tensor observation


def _stream(device: torch.device) -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _need_gpu(t, who: str) -> None:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise L.NativeLibraryError(f"{who} needs tensors on the GPU; fluidgym_amd has no CPU path")


def normalize_tensors(tensors: Sequence[torch.Tensor], means: Sequence[torch.Tensor], m2s: Sequence[torch.Tensor], rows: int, n_before: int,
                      *, pooled: bool = False, update: bool = True, row_list: Optional[torch.Tensor] = None, epsilon: float = 1e-8,
                      clip: Optional[float] = None) -> List[torch.Tensor]:
    """Every tensor of ``tensors`` (``rows`` contiguous rows each) normalised with its record ``means[j]``, ``m2s[j]`` (fp64 on the
    device, ``[D]`` or ``[1]`` pooled) as new tensors; with ``update`` the records are first advanced in place by the rows of
    ``row_list`` (ascending ``int32`` on the device; ``None``: all rows) and the caller adds that many rows to its ``n``.  One
    ``fg_obs_normalize`` call per 8 tensors, asynchronous on the current stream; there is no other path."""
    out: List[torch.Tensor] = []
    segs = []
    for t, mean, m2 in zip(tensors, means, m2s):
        _need_gpu(t, "the normalisation wrappers")
        if t.dtype not in _DTYPES or t.dtype != tensors[0].dtype:
            raise TypeError(f"the normalisation wrappers take float32 or float64 tensors of one dtype, got {t.dtype}")
        if t.numel() == 0 or t.numel() % rows:
            raise ValueError(f"a tensor of shape {tuple(t.shape)} does not hold {rows} rows")
        src = t.detach().contiguous()
        dst = torch.empty_like(src)
        n = src.numel() // rows
        for r in (mean, m2):
            if r.dtype != torch.float64 or r.device != src.device or not r.is_contiguous() or r.numel() != (1 if pooled else n):
                raise ValueError(f"a record of {tuple(r.shape)} {r.dtype} on {r.device} for rows of {n} elements (pooled: {pooled})")
        out.append(dst)
        segs.append((L.FgNormSegment(src.data_ptr(), dst.data_ptr(), n, n, n, 1 if pooled else 0, mean.data_ptr(), m2.data_ptr()), src))
    if not segs:
        return out
    lib = L.load()
    dev = tensors[0].device
    if row_list is not None and (row_list.device != dev or row_list.dtype != torch.int32 or not row_list.is_contiguous()):
        raise ValueError("row_list: a contiguous int32 tensor on the tensors' device")
    m = int(row_list.numel()) if row_list is not None else int(rows)
    rl = ctypes.c_void_p(row_list.data_ptr()) if row_list is not None else None
    for first in range(0, len(segs), MAX_SEGMENTS):
        chunk = segs[first: first + MAX_SEGMENTS]
        arr = (L.FgNormSegment * len(chunk))(*[s for s, _ in chunk])
        L.check(lib.fg_obs_normalize(arr, len(chunk), int(rows), _DTYPES[tensors[0].dtype], int(n_before), m if update else 0, rl,
                                     m if row_list is not None else 0, 1 if update else 0, float(epsilon),
                                     float(clip) if clip else 0.0, _stream(dev)))
    return out


def merge_records(n_a: int, mean_a: torch.Tensor, m2_a: torch.Tensor, n_b: int, mean_b: torch.Tensor, m2_b: torch.Tensor
                  ) -> Tuple[torch.Tensor, torch.Tensor]:
    """The Chan merge of two records in fp64 (counts in values, not rows): the update rule of this module with B in place of a batch."""
    if n_b == 0:
        return mean_a.clone(), m2_a.clone()
    if n_a == 0:
        return mean_b.clone().to(mean_a.device), m2_b.clone().to(m2_a.device)
    mean_b, m2_b = mean_b.to(mean_a.device), m2_b.to(m2_a.device)
    n = n_a + n_b
    delta = mean_b - mean_a
    return mean_a + delta * (n_b / n), m2_a + m2_b + (delta * delta) * (n_a * n_b / n)


class _RunningNormalizer(FluidWrapper):
    """What the two wrappers share: epsilon, clip, the row count ``n``, the update switch and the state entry."""

    _state_key = "normalizer"

    def __init__(self, env, epsilon: float, clip: Optional[float]) -> None:
        super().__init__(env)
        if not float(epsilon) > 0.0:
            raise ValueError("epsilon must be positive")
        if clip is not None and not float(clip) > 0.0:
            raise ValueError("clip must be positive (or None for no clip)")
        self._epsilon = float(epsilon)
        self._clip = None if clip is None else float(clip)
        self._n = 0
        self._updating = True

    # ---- the switch (the env's train() / val() / test() do not touch it)
    def freeze(self) -> None:
        """Stop updating the record: calls only normalise.  ``RuntimeError`` from the next call on while the record is empty."""
        self._updating = False

    def unfreeze(self) -> None:
        self._updating = True

    @property
    def updating(self) -> bool:
        return self._updating

    def _require_record(self) -> None:
        if self._n == 0:
            raise RuntimeError(f"{type(self).__name__}: the record is empty (n = 0) and cannot normalise; unfreeze() and update it, "
                               "or load() / merge() one")

    def _rstd(self, m2: torch.Tensor, count: int) -> torch.Tensor:
        return 1.0 / torch.sqrt(m2 / count + self._epsilon)

    def _record_device(self) -> torch.device:
        return torch.device(self._env.cuda_device)

    # ---- state: the inner state with this wrapper's record under a key of its own
    def _record_entry(self):
        raise NotImplementedError

    def _set_record_entry(self, entry) -> None:
        raise NotImplementedError

    def get_state(self):
        return push_state_entry(self._env.get_state(), self._state_key, self._record_entry(), type(self).__name__)

    def set_state(self, state) -> None:
        rest, entry = pop_state_entry(state, self._state_key, type(self).__name__)
        self._env.set_state(rest)
        self._set_record_entry(entry)


class NormalizeObservation(_RunningNormalizer):
    """Observations normalised by the running mean and variance of everything seen so far (module docstring).

    Parameters
    ----------
    env:
        The environment (or wrapper) to wrap: dict observations, or a single tensor (outside ``FlattenObservation``).
    epsilon: float
        Added to the variance under the square root.
    clip: float, optional
        The normalised values are clipped to ``[-clip, clip]``.
    pool: str
        ``"element"``: one record per element of a key's space; ``"key"``: one scalar record per key.
    keys: list of str, optional
        The keys to normalise (default: all); the others pass through untouched.
    """

    _state_key = "obs_normalizer"

    def __init__(self, env, epsilon: float = 1e-8, clip: Optional[float] = None, pool: str = "element",
                 keys: Optional[Sequence[str]] = None) -> None:
        super().__init__(env, epsilon, clip)
        if pool not in ("element", "key"):
            raise ValueError(f"pool must be 'element' or 'key', got {pool!r}")
        self._pooled = pool == "key"
        space = self._env.observation_space
        if isinstance(space, spaces.Dict):
            names = list(space.spaces) if keys is None else list(keys)
            for k in names:
                if k not in space.spaces:
                    raise ValueError(f"Key '{k}' not found in observation space.")
            self._keys: Optional[List[str]] = names
            subs = {k: space.spaces[k] for k in names}
        else:
            if keys is not None:
                raise ValueError("keys: only for Dict observation spaces")
            self._keys = None
            subs = {_SINGLE: space}
        self._sizes = {k: int(np.prod(s.shape, dtype=np.int64)) for k, s in subs.items()}
        self._mean: Dict[str, torch.Tensor] = {}
        self._m2: Dict[str, torch.Tensor] = {}
        bound = np.inf if self._clip is None else self._clip
        boxes = {k: spaces.Box(low=-bound, high=bound, shape=s.shape, dtype=s.dtype) for k, s in subs.items()}
        if self._keys is None:
            self._observation_space = boxes[_SINGLE]
        else:
            self._observation_space = spaces.Dict({k: boxes.get(k, s) for k, s in space.spaces.items()})

    @property
    def observation_space(self):
        return self._observation_space

    # ---- rows and records
    def _items(self, obs) -> List[Tuple[str, torch.Tensor, object]]:
        """(record key, tensor, space) of everything this wrapper normalises in ``obs``."""
        space = self._env.observation_space
        if self._keys is None:
            if isinstance(obs, dict):
                raise TypeError("NormalizeObservation: a dict observation where the space is a single Box")
            return [(_SINGLE, obs, space)]
        return [(k, obs[k], space.spaces[k]) for k in self._keys]

    @staticmethod
    def _rows_of(tensor: torch.Tensor, space) -> int:
        rows = 1
        for s in tensor.shape[: leading_dims(tensor, space)]:
            rows *= int(s)
        return rows

    def _ensure_records(self, device: torch.device) -> None:
        for k, size in self._sizes.items():
            if k not in self._mean:
                slots = 1 if self._pooled else size
                self._mean[k] = torch.zeros(slots, dtype=torch.float64, device=device)
                self._m2[k] = torch.zeros(slots, dtype=torch.float64, device=device)

    def _run(self, obs, update: bool, row_list: Optional[torch.Tensor] = None):
        if not update:
            self._require_record()
        items = self._items(obs)
        for _, t, _ in items:
            _need_gpu(t, "NormalizeObservation")
        rows = self._rows_of(items[0][1], items[0][2])
        self._ensure_records(items[0][1].device)
        done = normalize_tensors([t for _, t, _ in items], [self._mean[k] for k, _, _ in items], [self._m2[k] for k, _, _ in items], rows,
                                 self._n, pooled=self._pooled, update=update, row_list=row_list, epsilon=self._epsilon, clip=self._clip)
        if update:
            self._n += int(row_list.numel()) if row_list is not None else rows
        if self._keys is None:
            return done[0]
        new = dict(zip((k for k, _, _ in items), done))
        return {k: new.get(k, v) for k, v in obs.items()}

    # ---- the env surface
    def reset(self, seed: Optional[int] = None, randomize: Optional[bool] = None):
        if not self._updating:
            self._require_record()       # before the env moves and before any launch
        obs, info = self._env.reset(seed=seed, randomize=randomize)
        return self._run(obs, self._updating), info

    def reset_envs(self, envs, randomize: Optional[bool] = None):
        """The rows of the chosen envs update the record (the other rows of the batch are observations already counted); every row is
        normalised."""
        from ..simulation.state_bank import normalize_envs

        if not self._updating:
            self._require_record()       # before the env moves and before any launch
        obs = self._env.reset_envs(envs, randomize=randomize)
        if not self._updating:
            return self._run(obs, False)
        items = self._items(obs)
        _need_gpu(items[0][1], "NormalizeObservation")
        rows, num_envs = self._rows_of(items[0][1], items[0][2]), int(self._env.num_envs)
        per_env = rows // num_envs
        chosen = torch.as_tensor(sorted(normalize_envs(envs, num_envs)), dtype=torch.int32)
        row_list = (chosen[:, None] * per_env + torch.arange(per_env, dtype=torch.int32)[None, :]).reshape(-1).to(items[0][1].device)
        return self._run(obs, True, row_list)

    def step(self, action: torch.Tensor):
        if not self._updating:
            self._require_record()       # before the env moves and before any launch
        obs, reward, terminated, truncated, info = self._env.step(action)
        return self._run(obs, self._updating), reward, terminated, truncated, info

    # ---- the record applied by hand
    def normalize(self, obs):
        """``obs`` normalised with the current record, which is not updated (the frozen form of the kernel)."""
        return self._run(obs, False)

    def unnormalize(self, obs):
        """The inverse of ``normalize`` without the clip: ``y * sqrt(M2 / n + epsilon) + mean`` in fp64 (plain torch), rounded to the dtype."""
        self._require_record()
        done = {}
        for k, t, sp in self._items(obs):
            lead = leading_dims(t, sp)
            count = self._n * self._sizes[k] if self._pooled else self._n
            flat = t.reshape(tuple(t.shape[:lead]) + (-1,)).to(torch.float64)
            done[k] = (flat / self._rstd(self._m2[k], count) + self._mean[k]).to(t.dtype).reshape(t.shape)
        if self._keys is None:
            return done[_SINGLE]
        return {k: done.get(k, v) for k, v in obs.items()}

    @property
    def statistics(self) -> Dict[str, Tuple[int, torch.Tensor, torch.Tensor]]:
        """key -> ``(n, mean, var)``: the values merged (rows, or rows x D for ``pool="key"``), and clones of the mean and of ``M2 / n``."""
        out = {}
        for k, size in self._sizes.items():
            if k in self._mean:
                count = self._n * size if self._pooled else self._n
                out[k] = (count, self._mean[k].clone(), self._m2[k] / max(count, 1))
        return out

    def save(self, path) -> None:
        """The record as one ``.npz`` (host side: this synchronises)."""
        arrays = {"n": np.int64(self._n), "pooled": np.int64(self._pooled)}
        for k in self._mean:
            arrays["mean/" + k] = self._mean[k].cpu().numpy()
            arrays["M2/" + k] = self._m2[k].cpu().numpy()
        with open(path, "wb") as f:
            np.savez(f, **arrays)

    def load(self, path) -> None:
        with np.load(path) as z:
            if bool(z["pooled"]) != self._pooled:
                raise ValueError("NormalizeObservation.load: the file's record was kept with another pool")
            entry = {"n": int(z["n"]), "mean": {}, "M2": {}}
            for name in z.files:
                if name.startswith("mean/"):
                    entry["mean"][name[5:]] = torch.from_numpy(z[name])
                    entry["M2"][name[5:]] = torch.from_numpy(z["M2/" + name[5:]])
        self._set_record_entry(entry)

    def merge(self, other: "NormalizeObservation") -> None:
        """The Chan merge of ``other``'s record into this one, in fp64, for shards wrapped separately (host-side logic on the records'
        tensors, not a kernel)."""
        if not isinstance(other, NormalizeObservation) or other._pooled != self._pooled or other._sizes != self._sizes:
            raise ValueError("NormalizeObservation.merge: the other record has another pool, other keys or other sizes")
        if other._n == 0:
            return
        self._ensure_records(next(iter(self._mean.values())).device if self._mean else next(iter(other._mean.values())).device)
        for k, size in self._sizes.items():
            scale = size if self._pooled else 1
            self._mean[k], self._m2[k] = merge_records(self._n * scale, self._mean[k], self._m2[k], other._n * scale, other._mean[k],
                                                       other._m2[k])
        self._n += other._n

    def _record_entry(self):
        return {"n": self._n, "mean": {k: v.clone() for k, v in self._mean.items()}, "M2": {k: v.clone() for k, v in self._m2.items()}}

    def _set_record_entry(self, entry) -> None:
        slots = {k: 1 if self._pooled else size for k, size in self._sizes.items()}
        for k in entry["mean"]:
            if k not in slots or entry["mean"][k].numel() != slots[k] or entry["M2"][k].numel() != slots[k]:
                raise ValueError(f"NormalizeObservation: the record of '{k}' does not fit this wrapper's keys and pool")
        dev = self._record_device()
        self._n = int(entry["n"])
        self._mean = {k: v.clone().to(dev, torch.float64).contiguous() for k, v in entry["mean"].items()}
        self._m2 = {k: v.clone().to(dev, torch.float64).contiguous() for k, v in entry["M2"].items()}


class NormalizeReward(_RunningNormalizer):
    """Rewards scaled by the running standard deviation of the discounted return ``G[r] = gamma * G[r] + reward[r]`` kept per row of the
    reward (``[B]``, ``[B, n_agents]``; an un-batched single-agent env is one row): ``reward / sqrt(var(G) + epsilon)``, no mean
    subtraction, as gymnasium does.  One scalar record over every ``G`` value produced; ``reset()`` zeroes every ``G``,
    ``reset_envs(envs)`` the rows of the chosen envs.  One ``fg_obs_return_normalize`` launch per step.

    Parameters
    ----------
    env:
        The environment (or wrapper) to wrap.
    gamma: float
        The discount of the return, in [0, 1].
    epsilon: float
        Added to the variance under the square root.
    clip: float, optional
        The scaled rewards are clipped to ``[-clip, clip]``.
    """

    _state_key = "reward_normalizer"

    def __init__(self, env, gamma: float = 0.99, epsilon: float = 1e-8, clip: Optional[float] = None) -> None:
        super().__init__(env, epsilon, clip)
        if not 0.0 <= float(gamma) <= 1.0:
            raise ValueError("gamma must lie in [0, 1]")
        self._gamma = float(gamma)
        self._G: Optional[torch.Tensor] = None          # fp64 [rows]
        self._stats: Optional[torch.Tensor] = None      # fp64 {mean, M2}

    @property
    def returns(self) -> Optional[torch.Tensor]:
        """The discounted returns ``G`` (fp64 ``[rows]``; None before the first step)."""
        return self._G

    def _ensure_stats(self, device: torch.device) -> torch.Tensor:
        if self._stats is None:
            self._stats = torch.zeros(2, dtype=torch.float64, device=device)
        return self._stats

    def reset(self, seed: Optional[int] = None, randomize: Optional[bool] = None):
        out = self._env.reset(seed=seed, randomize=randomize)
        if self._G is not None:
            self._G.zero_()
        return out

    def reset_envs(self, envs, randomize: Optional[bool] = None):
        from ..simulation.state_bank import normalize_envs

        obs = self._env.reset_envs(envs, randomize=randomize)
        if self._G is not None:
            num_envs = int(self._env.num_envs)
            chosen = torch.as_tensor(normalize_envs(envs, num_envs), dtype=torch.int64, device=self._G.device)
            self._G.view(num_envs, -1)[chosen] = 0.0
        return obs

    def step(self, action: torch.Tensor):
        if not self._updating:
            self._require_record()       # before the env moves and before any launch
        obs, reward, terminated, truncated, info = self._env.step(action)
        _need_gpu(reward, "NormalizeReward")
        if reward.dtype not in _DTYPES:
            raise TypeError(f"NormalizeReward takes float32 or float64 rewards, got {reward.dtype}")
        src = reward.detach().contiguous()
        rows = int(src.numel())
        if self._G is None:
            self._G = torch.zeros(rows, dtype=torch.float64, device=src.device)
        elif self._G.numel() != rows:
            raise ValueError(f"NormalizeReward: a reward of {rows} rows where the returns hold {self._G.numel()}")
        stats = self._ensure_stats(src.device)
        out = torch.empty_like(src)
        p = ctypes.c_void_p
        L.check(L.load().fg_obs_return_normalize(p(src.data_ptr()), p(out.data_ptr()), p(self._G.data_ptr()), p(stats.data_ptr()), rows,
                                                 _DTYPES[src.dtype], self._gamma, self._n, self._epsilon, self._clip or 0.0,
                                                 1 if self._updating else 0, _stream(src.device)))
        if self._updating:
            self._n += rows
        return obs, out, terminated, truncated, info

    # ---- the record applied by hand
    def _scale(self) -> torch.Tensor:
        self._require_record()
        return self._rstd(self._stats[1], self._n)

    def normalize(self, reward: torch.Tensor) -> torch.Tensor:
        """``reward`` scaled (and clipped) with the current record; neither the record nor ``G`` moves (plain torch, fp64)."""
        y = reward.to(torch.float64) * self._scale().to(reward.device)
        if self._clip is not None:
            y = y.clamp(-self._clip, self._clip)
        return y.to(reward.dtype)

    def unnormalize(self, reward: torch.Tensor) -> torch.Tensor:
        return (reward.to(torch.float64) / self._scale().to(reward.device)).to(reward.dtype)

    @property
    def statistics(self) -> Tuple[int, torch.Tensor, torch.Tensor]:
        """``(n, mean, var)`` of the returns merged so far."""
        stats = self._ensure_stats(self._record_device())
        return self._n, stats[0].clone(), stats[1] / max(self._n, 1)

    def save(self, path) -> None:
        """The record as one ``.npz`` (host side: this synchronises).  ``G`` belongs to the running episodes and is not part of it."""
        stats = self._ensure_stats(self._record_device())
        with open(path, "wb") as f:
            np.savez(f, n=np.int64(self._n), stats=stats.cpu().numpy())

    def load(self, path) -> None:
        with np.load(path) as z:
            self._n = int(z["n"])
            self._stats = torch.from_numpy(z["stats"]).to(self._record_device(), torch.float64).contiguous()

    def merge(self, other: "NormalizeReward") -> None:
        """The Chan merge of ``other``'s record into this one, in fp64 (host-side logic, not a kernel)."""
        if not isinstance(other, NormalizeReward):
            raise ValueError("NormalizeReward.merge: not a NormalizeReward")
        if other._n == 0:
            return
        mine = self._ensure_stats(other._stats.device if self._stats is None else self._stats.device)
        mean, m2 = merge_records(self._n, mine[0], mine[1], other._n, other._stats[0], other._stats[1])
        self._stats = torch.stack([mean, m2])
        self._n += other._n

    def _record_entry(self):
        stats = self._stats
        return {"n": self._n, "mean": None if stats is None else stats[0].clone(), "M2": None if stats is None else stats[1].clone(),
                "G": None if self._G is None else self._G.clone()}

    def _set_record_entry(self, entry) -> None:
        self._n = int(entry["n"])
        self._stats = None if entry["mean"] is None else torch.stack([entry["mean"], entry["M2"]]).to(torch.float64).contiguous()
        self._G = None if entry["G"] is None else entry["G"].clone()
