"""``StateBank``: stored domain states that chosen envs of a batch are restored from (``Domain.RestoreEnvs``,
``FluidEnv.reset_envs``), and the host side of the selection records the restore kernel reads (``csrc/fg_envrestore.hip``).

A bank holds ``S`` states as ``[S, ...]`` device tensors, one per field that ``Domain.Clone()`` snapshots: velocity, pressure,
passive scalar, velocity source and the boundary arrays of the FIXED faces.  A restore copies state ``src`` into env ``env``, mirrored
and then rolled along the periodic axes -- ``torch.roll(torch.flip(t, [-1]), shift, -1)`` with the sign change of the mirrored
velocity component, the reference's batch-wide randomisation (``rbc_env_base.py:335-362``) with one decision per env.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from .. import _lib as L

SYMMETRIES = ("flip_x", "flip_z", "shift_x", "shift_z")       # the order they are drawn in (the reference's: mirrors, then rolls)


def normalize_envs(envs, batch: int) -> List[int]:
    """``envs`` -- a sequence of indices or a bool mask ``[batch]`` -- as an ascending list.  ``ValueError``: an index out of range, an
    env named twice, a mask of another length, nothing chosen."""
    a = envs.detach().cpu().numpy() if isinstance(envs, torch.Tensor) else np.asarray(envs)
    if a.dtype == np.bool_:
        if a.shape != (batch,):
            raise ValueError(f"envs: a bool mask needs shape ({batch},), got {a.shape}")
        a = np.nonzero(a)[0]
    a = a.reshape(-1)
    if a.size == 0:
        raise ValueError("envs: nothing chosen")
    if not np.issubdtype(a.dtype, np.integer):
        raise ValueError("envs: indices or a bool mask")
    out = sorted(int(i) for i in a)
    if out[0] < 0 or out[-1] >= batch:
        raise ValueError(f"envs: an index is outside [0, {batch})")
    if len(set(out)) != len(out):
        raise ValueError("envs: an env is named twice")
    return out


def _per_env(v, n: int, what: str) -> List[int]:
    if v is None:
        return [0] * n
    a = np.asarray(v.detach().cpu() if isinstance(v, torch.Tensor) else v).reshape(-1)
    if a.size == 1:
        a = np.repeat(a, n)
    if a.size != n:
        raise ValueError(f"{what}: one value or one per chosen env ({n}), got {a.size}")
    return [int(x) for x in a]


def build_selection(envs: Sequence[int], src, flip_x=None, flip_z=None, shift_x=None, shift_z=None, *, batch: int, n_states: int,
                    dims: int, nx: int, nz: int = 1, periodic_x: bool = True, periodic_z: bool = False):
    """The ``fg_env_sel`` records of a restore as a ctypes array; refuses (``ValueError``) what ``fg_env_restore_field`` refuses: more
    records than envs, an env or source index out of range, an env named twice, a flip that is not 0 / 1, a shift outside
    ``[0, n)``, a flip or roll along an axis that is not periodic, ``flip_z`` / ``shift_z`` on a 2-D grid."""
    envs = [int(e) for e in (envs.tolist() if isinstance(envs, (np.ndarray, torch.Tensor)) else envs)]
    n = len(envs)
    if n < 1 or n > batch:
        raise ValueError(f"selection: between 1 and {batch} envs, got {n}")
    cols = [_per_env(src, n, "src"), _per_env(flip_x, n, "flip_x"), _per_env(flip_z, n, "flip_z"),
            _per_env(shift_x, n, "shift_x"), _per_env(shift_z, n, "shift_z")]
    seen = set()
    sel = (L.FgEnvSel * n)()
    for i, (e, s, fx, fz, sx, sz) in enumerate(zip(envs, *cols)):
        if not 0 <= e < batch:
            raise ValueError(f"selection: env {e} is outside [0, {batch})")
        if e in seen:
            raise ValueError(f"selection: env {e} is named twice")
        seen.add(e)
        if not 0 <= s < n_states:
            raise ValueError(f"selection: source state {s} is outside [0, {n_states})")
        if fx not in (0, 1) or fz not in (0, 1):
            raise ValueError("selection: a flip is 0 or 1")
        if dims == 2 and (fz or sz):
            raise ValueError("selection: flip_z / shift_z on a 2-D grid")
        if not 0 <= sx < nx or not 0 <= sz < max(nz, 1):
            raise ValueError("selection: a shift must be in [0, n)")
        if not periodic_x and (fx or sx):
            raise ValueError("selection: flip / roll along x, which is not periodic")
        if dims == 3 and not periodic_z and (fz or sz):
            raise ValueError("selection: flip / roll along z, which is not periodic")
        sel[i] = L.FgEnvSel(e, s, fx, fz, sx, sz)
    return sel


def draw_reset_plan(rng: np.random.Generator, envs: Sequence[int], n_states: int, symmetries: Sequence[str], nx: int, nz: int = 1,
                    randomize: bool = True) -> Dict[str, List[int]]:
    """What ``reset_envs`` draws from the env's NumPy generator: for each chosen env in ascending index order the source state
    (``integers(0, n_states)``, only when the bank holds more than one) and then the env family's symmetries in the order of
    ``SYMMETRIES`` -- a mirror is ``uniform(0, 1) > 0.5``, a roll ``integers(0, n)``, as the reference draws them for the batch
    (``rbc_env_base.py:338-362``).  Without ``randomize`` nothing is drawn: state 0, no mirror, no roll."""
    unknown = set(symmetries) - set(SYMMETRIES)
    if unknown:
        raise ValueError(f"unknown symmetries {sorted(unknown)}; known: {SYMMETRIES}")
    plan: Dict[str, List[int]] = {"env": [], "src": [], **{k: [] for k in SYMMETRIES}}
    for e in sorted(int(i) for i in envs):
        plan["env"].append(e)
        plan["src"].append(int(rng.integers(0, n_states)) if (randomize and n_states > 1) else 0)
        for k in SYMMETRIES:
            if not randomize or k not in symmetries:
                plan[k].append(0)
            elif k.startswith("flip"):
                plan[k].append(int(rng.uniform(0.0, 1.0) > 0.5))
            else:
                plan[k].append(int(rng.integers(0, nx if k == "shift_x" else nz)))
    return plan


class StateBank:
    """``S`` stored states of one domain layout.

    ``states``: ``Domain.Clone()`` / ``get_state()["domain"]`` dicts (or whole ``get_state()`` dicts).  With ``env=k`` env ``k`` of
    each is taken; without it every env of every dict is an entry of its own, in order.  The ``solver_hints`` of a snapshot belong
    to a solver handle, not to a state, and are not kept."""

    def __init__(self, states: Sequence[dict], env: Optional[int] = None):
        states = [s["domain"] if "domain" in s else s for s in states]
        if not states:
            raise ValueError("StateBank: no states")
        pick = (lambda t: t) if env is None else (lambda t: t[int(env): int(env) + 1])
        stack = lambda ts: torch.cat([pick(t) for t in ts], dim=0).contiguous()
        keys = [k for k in ("velocity", "pressure", "scalar", "velocity_source") if k in states[0]]
        for s in states:
            if [k for k in ("velocity", "pressure", "scalar", "velocity_source") if k in s] != keys:
                raise ValueError("StateBank: the states do not hold the same fields")
        self.fields: Dict[str, torch.Tensor] = {k: stack([s[k] for s in states]) for k in keys}
        self.bvel: Dict[int, torch.Tensor] = {int(f): stack([s["bvel"][f] for s in states]) for f in states[0].get("bvel", {})}
        self.bscal: Dict[int, torch.Tensor] = {int(f): stack([s["bscal"][f] for s in states]) for f in states[0].get("bscal", {})}

    @property
    def size(self) -> int:
        return int(self.fields["velocity"].shape[0])

    def __len__(self) -> int:
        return self.size
