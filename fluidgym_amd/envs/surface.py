"""Surface curves of the cylinder and airfoil envs: the pressure coefficient ``Cp``, the skin friction ``Cf`` and the traction along
the wall ring, with the coordinates an aerodynamicist plots them against, and the separation points.

The reference reduces the wall to drag and lift (``_get_drag_and_lift``, ``cylinder_env_base.py:616-700``); the integrand of that
sum is ``WallRing.distribution`` here (one launch of ``fg_mb_wall_distribution``), and ``SurfaceDistribution`` is that integrand with
its normalisation ``q = U_mean^2 / 2`` -- the dynamic pressure ``_get_drag_and_lift`` divides by -- and the geometry of the ring.
Everything stays on the device; ``separation_points`` reads ``cf`` back, since its answer has a different length per env."""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Union

import numpy as np
import torch


def separation_points(cf, arc_length, perimeter: float) -> List[np.ndarray]:
    """Per env the positions along the ring (same unit and origin as ``arc_length``, ascending) where ``cf [B, n]`` (or ``[n]``: one
    env) changes sign between neighbouring faces: a crossing is linearly interpolated between the two face midpoints, and the step from
    the last face back to the first counts (its far end lies at ``arc_length[0] + perimeter``; a crossing beyond the perimeter is
    wrapped).  A face whose ``cf`` is exactly zero counts as positive."""
    v = np.asarray(cf.detach().cpu() if isinstance(cf, torch.Tensor) else cf, np.float64)
    v = v[None] if v.ndim == 1 else v
    s = np.asarray(arc_length.detach().cpu() if isinstance(arc_length, torch.Tensor) else arc_length, np.float64)
    if v.ndim != 2 or s.shape != (v.shape[1],):
        raise ValueError(f"separation_points: cf must be [B, n] and arc_length [n], got {v.shape} and {s.shape}")
    s_next = np.concatenate([s[1:], [s[0] + float(perimeter)]])
    out = []
    for row in v:
        nxt = np.roll(row, -1)
        at = np.nonzero((row >= 0) != (nxt >= 0))[0]
        t = row[at] / (row[at] - nxt[at])
        out.append(np.sort(np.mod(s[at] + t * (s_next[at] - s[at]), float(perimeter))))
    return out


def ring_theta(face_centers: np.ndarray, vertices: np.ndarray) -> np.ndarray:
    """Degrees about the centroid of the ring's vertices, from the upstream direction (``-x``), counter-clockwise, in (-180, 180]."""
    c = np.asarray(vertices, np.float64)[:, :-1].mean(axis=1, keepdims=True)
    d = np.asarray(face_centers, np.float64) - c
    th = np.degrees(np.arctan2(d[1], d[0])) - 180.0
    return np.where(th <= -180.0, th + 360.0, th)


def ring_chord_coordinates(face_centers: np.ndarray, vertices: np.ndarray, normals: np.ndarray):
    """``(x_over_c, side)`` of an airfoil ring: the face midpoints between the minimum and maximum ``x`` of the ring's vertices, and
    +1 (the normal into the fluid points up) or -1 per face."""
    x = np.asarray(vertices, np.float64)[0]
    x_over_c = (np.asarray(face_centers, np.float64)[0] - x.min()) / (x.max() - x.min())
    return x_over_c, np.where(np.asarray(normals, np.float64)[1] >= 0, 1.0, -1.0)


@dataclass
class SurfaceDistribution:
    """One instant of the wall curves of a batch, on the device.  ``p``, ``tau_w``, ``cp``, ``cf``: ``[B, n]``, in 3-D ``[B, nz, n]``;
    ``traction``: ``[B, 2, ...]``; the coordinates ``[n]`` (``face_centers [2, n]``).  Cylinders carry ``theta`` (degrees about the
    ring centroid from the upstream direction, counter-clockwise, in (-180, 180]), airfoils ``x_over_c`` and ``side`` (+1 upper,
    -1 lower); the other family's fields are None."""
    p: torch.Tensor
    tau_w: torch.Tensor
    traction: torch.Tensor
    cp: torch.Tensor
    cf: torch.Tensor
    arc_length: torch.Tensor
    face_centers: torch.Tensor
    face_lengths: torch.Tensor
    perimeter: float
    q: float                            # U_mean^2 / 2
    layer_height: float = 1.0           # spanwise height of a layer (3-D)
    theta: Optional[torch.Tensor] = None
    x_over_c: Optional[torch.Tensor] = None
    side: Optional[torch.Tensor] = None

    def forces(self, layer_height: Optional[float] = None) -> torch.Tensor:
        """The traction integrated with the face lengths: ``[B, 2]``, per spanwise layer ``[B, 2, nz]`` in 3-D (face area = length x
        ``layer_height``, default the env's) -- what ``WallRing.forces`` sums inside its kernel."""
        if self.traction.ndim == 3:
            return (self.traction * self.face_lengths).sum(-1)
        h = self.layer_height if layer_height is None else float(layer_height)
        return (self.traction * (self.face_lengths * h)).sum(-1)

    def separation_points(self, cf=None) -> List[np.ndarray]:
        """Per env the arc lengths where ``cf`` (default: this instant's, in 3-D its span average; any ``[B, n]`` curve such as a
        time mean is taken) changes sign along the ring: see :func:`separation_points`."""
        cf = self.cf if cf is None else cf
        if isinstance(cf, torch.Tensor) and cf.ndim == 3:
            cf = cf.mean(dim=1)
        return separation_points(cf, self.arc_length, self.perimeter)


class SurfaceMixin:
    """``get_surface_distribution`` of the envs with a wall ring (``self._ring``; cylinder and airfoil families)."""

    _wall_family = "cylinder"           # which coordinate the curves carry: "cylinder" (theta) or "airfoil" (x_over_c, side)

    def _wall_force_args(self):
        """``(viscosity, layer_height)`` as ``_get_drag_and_lift`` hands them to ``WallRing.forces``."""
        raise NotImplementedError

    def _surface_coordinates(self) -> dict:
        cached = self.__dict__.get("_surface_coords")
        ring = self._ring
        if cached is None or cached[0] is not ring:
            dev = self._domain.device
            t = lambda v: torch.as_tensor(np.ascontiguousarray(v), dtype=torch.float64, device=dev)
            v = ring.vertices.numpy()
            perimeter = float(np.sqrt(((v[:, 1:] - v[:, :-1]) ** 2).sum(0)).sum())
            coords = dict(arc_length=t(ring.arc_length), face_centers=t(ring.face_centers), perimeter=perimeter)
            if self._wall_family == "airfoil":
                x_over_c, side = ring_chord_coordinates(ring.face_centers, v, ring.wall_normals.cpu().numpy())
                coords.update(x_over_c=t(x_over_c), side=t(side))
            else:
                coords.update(theta=t(ring_theta(ring.face_centers, v)))
            cached = self._surface_coords = (ring, coords)
        return cached[1]

    def get_surface_distribution(self, p_ref: Union[float, torch.Tensor] = 0.0) -> SurfaceDistribution:
        """The wall curves of every env from the current fields, in one launch: ``p``, ``tau_w``, the traction,
        ``cp = (p - p_ref) / q`` and ``cf = tau_w / q`` with ``q = U_mean^2 / 2``.  ``p_ref``: a float or one value per env (``[B]``
        tensor); 0, the default, is the solver's own gauge -- the pressure field is kept mean-free over the domain -- and not the
        free-stream pressure, so pass the pressure of an upstream probe for the textbook ``Cp``."""
        if getattr(self, "_domain", None) is None or getattr(self, "_ring", None) is None:
            raise RuntimeError("get_surface_distribution: reset() the env first (the domain does not exist yet)")
        nu, layer_height = self._wall_force_args()
        ring, dom = self._ring, self._domain
        d = ring.distribution(dom, nu)                          # [B, 4, layers, n]
        if ring.dims == 2:
            d = d[:, :, 0]
        q = 0.5 * float(self._U_mean) ** 2
        p, tau = d[:, 0], d[:, 1]
        if isinstance(p_ref, torch.Tensor):
            if p_ref.numel() not in (1, p.shape[0]):
                raise ValueError(f"p_ref must be a float or one value per env ({p.shape[0]})")
            ref = p_ref.detach().to(device=p.device, dtype=p.dtype).reshape((-1,) + (1,) * (p.ndim - 1))
        else:
            ref = float(p_ref)
        return SurfaceDistribution(p=p, tau_w=tau, traction=d[:, 2:4], cp=(p - ref) / q, cf=tau / q,
                                   face_lengths=ring.face_lengths.to(device=p.device, dtype=p.dtype), q=q,
                                   layer_height=float(layer_height) if ring.dims == 3 else 1.0,
                                   **self._surface_coordinates())
