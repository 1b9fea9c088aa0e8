"""Space helpers of the wrappers (reference ``fluidgym/wrappers/util.py``), on ``fluidgym_amd.spaces``."""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np
import torch

from .. import spaces


def flatten_box_space(space: spaces.Box) -> spaces.Box:
    """The 1-D ``Box`` with the flattened bounds of ``space``."""
    return spaces.Box(low=space.low.flatten(), high=space.high.flatten(), dtype=space.dtype)


def flatten_dict_space(space: spaces.Dict, keys: Optional[List[str]] = None) -> spaces.Box:
    """One 1-D ``Box`` of the ``Box`` subspaces ``keys`` of a ``Dict`` (default: all, in the dict's order), bounds concatenated;
    its dtype is the common type of the subspaces and float32."""
    if not isinstance(space, spaces.Dict):
        raise TypeError(f"Expected spaces.Dict, got {type(space)}")
    if keys is None:
        items = list(space.spaces.items())
    else:
        for k in keys:
            if k not in space.spaces:
                raise KeyError(f"Key '{k}' not found in the Dict space.")
        items = [(k, space.spaces[k]) for k in keys]
    lows, highs, dtypes = [], [], []
    for k, sub in items:
        if not isinstance(sub, spaces.Box):
            raise TypeError(f"Only Box subspaces supported, but key '{k}' is {type(sub)}")
        lows.append(np.asarray(sub.low).reshape(-1))
        highs.append(np.asarray(sub.high).reshape(-1))
        dtypes.append(sub.dtype)
    if not lows:
        raise ValueError("Dict space contains no Box subspaces to flatten.")
    dtype = np.result_type(*dtypes, np.float32)
    return spaces.Box(low=np.concatenate(lows).astype(dtype, copy=False), high=np.concatenate(highs).astype(dtype, copy=False), dtype=dtype)


def leading_dims(tensor: torch.Tensor, space) -> int:
    """How many leading axes (env axis, agent axis) ``tensor`` carries in front of one item of ``space``: ``dim()`` minus the rank of the
    space.  0 for an un-batched single-agent env, 1 for ``[B, ...]`` or ``[n_agents, ...]``, 2 for ``[B, n_agents, ...]``."""
    rank = len(space.shape)
    lead = tensor.dim() - rank
    if lead < 0 or tuple(tensor.shape[lead:]) != tuple(space.shape):
        raise ValueError(f"a tensor of shape {tuple(tensor.shape)} does not end in the shape {tuple(space.shape)} of its space")
    return lead


def numbered_state_keys(state: dict, key: str) -> List[str]:
    """The entries ``key``, ``key#1``, ``key#2``, ... that ``state`` holds, in that order: wrappers of one kind nested in each other
    keep their ``get_state()`` entries apart by number, the innermost taking the bare key."""
    keys, i = [], 0
    while (key if i == 0 else f"{key}#{i}") in state:
        keys.append(key if i == 0 else f"{key}#{i}")
        i += 1
    return keys


def push_state_entry(inner, key: str, value, who: str) -> dict:
    """A copy of the wrapped env's state ``inner`` with ``value`` under the next free number of ``key``."""
    if not isinstance(inner, dict):
        raise TypeError(f"{who}.get_state: the wrapped env's state is not a dict")
    state = dict(inner)
    taken = len(numbered_state_keys(state, key))       # wrappers of this kind further in took the lower numbers
    state[key if taken == 0 else f"{key}#{taken}"] = value
    return state


def pop_state_entry(state, key: str, who: str) -> Tuple[dict, object]:
    """``(rest, value)``: the highest-numbered ``key`` entry of ``state`` -- the outermost wrapper's -- and the state without it."""
    mine = numbered_state_keys(state, key)
    if not mine:
        raise KeyError(f"{who}.set_state: the state holds no '{key}' entry")
    rest = dict(state)
    return rest, rest.pop(mine[-1])
