"""``MeshStateBank``: stored states of a multi-block domain that chosen envs of a batch are restored from
(``MultiBlockDomain.RestoreEnvs``, ``reset_mesh_envs`` of the cylinder and airfoil envs; ``csrc/fg_mb_envrestore.hip``), and
``span_symmetry``, which says whether a mesh is an equal-layer prism along z -- the condition under which a mirror and a roll along
the span map a state of the mesh onto a state of it.

A ``MultiBlockDomain`` carries three per-env arrays between steps (``Clone()``): ``velocity [B, d, N]``, ``pressure [B, N]`` and
``boundary_velocity [B, d, NB]``; a bank holds ``S`` of each as ``[S, ...]`` device tensors.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np
import torch

FIELDS = ("velocity", "pressure", "boundary_velocity")


class MeshStateBank:
    """``S`` stored states of one multi-block mesh.

    ``states``: ``MultiBlockDomain.Clone()`` / ``get_state()["domain"]`` dicts (or whole ``get_state()`` dicts).  With ``env=k`` env
    ``k`` of each is taken; without it every env of every dict is an entry of its own, in order.  The ``solver_hints`` of a snapshot
    belong to a solver handle, not to a state, and are not kept."""

    def __init__(self, states: Sequence[dict], env: Optional[int] = None):
        states = [s["domain"] if "domain" in s else s for s in states]
        if not states:
            raise ValueError("MeshStateBank: no states")
        for s in states:
            missing = [k for k in FIELDS if k not in s]
            if missing:
                raise ValueError(f"MeshStateBank: a state lacks {missing} (a MultiBlockDomain.Clone() holds {list(FIELDS)})")
        first = states[0]
        for s in states:
            for k in FIELDS:
                if tuple(s[k].shape[1:]) != tuple(first[k].shape[1:]) or s[k].dtype != first[k].dtype or s[k].device != first[k].device:
                    raise ValueError(f"MeshStateBank: the states do not hold the same fields: {k} is {tuple(s[k].shape[1:])} {s[k].dtype} "
                                     f"on {s[k].device} in one and {tuple(first[k].shape[1:])} {first[k].dtype} on {first[k].device} in another")
            if len({int(s[k].shape[0]) for k in FIELDS}) != 1:
                raise ValueError("MeshStateBank: the fields of a state differ in their batch size")
            if env is not None and not 0 <= int(env) < int(s["velocity"].shape[0]):
                raise ValueError(f"MeshStateBank: env {env} is outside a state's batch of {int(s['velocity'].shape[0])}")
        pick = (lambda t: t) if env is None else (lambda t: t[int(env): int(env) + 1])
        self.fields: Dict[str, torch.Tensor] = {k: torch.cat([pick(s[k]) for s in states], dim=0).contiguous() for k in FIELDS}

    @property
    def size(self) -> int:
        return int(self.fields["velocity"].shape[0])

    def __len__(self) -> int:
        return self.size


def span_symmetry(coords_list, periodic_z) -> Optional[int]:
    """``nz`` when the mesh ``coords_list`` (one vertex array ``[3, nz+1, ny+1, nx+1]`` per block; ``periodic_z``: one bool per block)
    is an equal-layer prism along z, else None.  Pure NumPy.  The conditions:

    * 3-D, every block z-periodic, one ``nz``;
    * x and y of every vertex equal in every layer, bit for bit, and z one value per layer, the same in every block;
    * layer spacings equal within 8 ulp of ``max|z|`` in the mesh's dtype (``extrude_mesh`` forms z from two rounded products and a
      sum: about 3 ulp between spacings; 8 leaves headroom).  The mesh's dtype is that of the arrays, or float32 when every
      coordinate of a float64 array is a float32 value (a float64 domain built from a float32 mesh)."""
    coords_list = [np.asarray(c) for c in coords_list]
    periodic_z = list(periodic_z)
    if not coords_list or len(periodic_z) != len(coords_list):
        return None
    if any(c.ndim != 4 or c.shape[0] != 3 for c in coords_list) or not all(bool(p) for p in periodic_z):
        return None
    nz = coords_list[0].shape[1] - 1
    if nz < 1 or any(c.shape[1] - 1 != nz for c in coords_list):
        return None
    z = coords_list[0][2, :, 0, 0]
    for c in coords_list:
        if not (np.array_equal(c[:2], np.broadcast_to(c[:2, :1], c[:2].shape))
                and np.array_equal(c[2], np.broadcast_to(z[:, None, None].astype(c.dtype), c[2].shape))):
            return None
    dtype = np.result_type(*[c.dtype for c in coords_list])
    if dtype == np.float64 and all(np.array_equal(c.astype(np.float32).astype(np.float64), c) for c in coords_list):
        dtype = np.dtype(np.float32)
    if dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
        return None
    z = z.astype(dtype)
    dz = np.diff(z)
    if not np.all(np.isfinite(dz)) or not np.all(dz > 0):
        return None
    tol = 8.0 * float(np.spacing(np.abs(z).max().astype(dtype)))
    return int(nz) if float(dz.max()) - float(dz.min()) <= tol else None
