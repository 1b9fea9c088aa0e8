"""Host plumbing shared by the online plane recorders (``plane_stats``, ``plane_spectra``, ``plane_budgets``, ``plane_timecorr``):
the channel views of a domain's tensors, the checks of fields that go to the GPU, the pointer and stride tables of the
``fg_plane_*`` entry points, the library of a dtype, the device-resident state of an accumulator and the wall units of a record
with a mean-``u`` profile."""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from .. import _lib as L


def gather(channels, velocity, pressure, scalar, what: str, *, pressure_required: bool = False, w_exact: bool = False):
    """(tensor, component) of every channel: views of the domain's ``[B, C, (Z,) Y, X]`` tensors (NumPy or torch).
    ``pressure_required``: a pressure on the velocity's grid is demanded even when no channel reads it; ``w_exact``: the channels
    hold ``w`` exactly when the velocity has three components (otherwise ``w`` merely needs a third component)."""
    if velocity.ndim not in (4, 5):
        raise ValueError(f"{what}: velocity must be [B, d, (Z,) Y, X]; multi-block domains (flat [B, d, N] fields) are not supported")
    d = velocity.shape[1]
    if d != velocity.ndim - 2 or (("w" in channels) != (d == 3) if w_exact else ("w" in channels and d != 3)):
        raise ValueError(f"{what}: channels {channels} do not fit a velocity of shape {tuple(velocity.shape)}")
    if (pressure_required or "p" in channels) and (pressure is None
                                                   or tuple(pressure.shape) != (velocity.shape[0], 1) + tuple(velocity.shape[2:])):
        raise ValueError(f"{what}: pressure must be [B, 1, (Z,) Y, X] on the velocity's grid")
    if "T" in channels and (scalar is None or scalar.ndim != velocity.ndim or tuple(scalar.shape[2:]) != tuple(velocity.shape[2:])
                            or scalar.shape[0] != velocity.shape[0]):
        raise ValueError(f"{what}: channel T needs the passive scalar [B, S, (Z,) Y, X]")
    src = {"u": (velocity, 0), "v": (velocity, 1), "w": (velocity, 2), "p": (pressure, 0), "T": (scalar, 0)}
    return [src[c] for c in channels]


def check_device_fields(fields, what: str, host_twin: str) -> None:
    """``fields`` (the velocity first) are GPU tensors of one dtype and device, float32 or float64."""
    first = fields[0]
    for t in fields:
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise ValueError(f"{what}: the fields must be tensors on the GPU ({host_twin} takes host arrays)")
        if t.dtype != first.dtype or t.device != first.device:
            raise TypeError(f"{what}: all fields need one dtype and device")
    if first.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"{what}: float32 or float64 fields, got {first.dtype}")


def grid_of(velocity):
    """``(B, nz, ny, nx)`` of a velocity ``[B, d, (Z,) Y, X]``; ``nz = 1`` in 2-D."""
    return (int(velocity.shape[0]),) + ((1,) + tuple(int(s) for s in velocity.shape[2:]))[-3:]


def channel_table(parts, cells: int):
    """The pointer and batch-stride tables of ``parts``, contiguous ``[B, C, ...]`` tensors with the component to read of each."""
    ptrs = (ctypes.c_void_p * len(parts))(*[t.data_ptr() + c * cells * t.element_size() for t, c in parts])
    strides = (ctypes.c_int64 * len(parts))(*[int(t.shape[1]) * cells for t, _ in parts])
    return ptrs, strides


def library(dtype):
    """float32 -> ``libfluidgym_hip.so``, float64 -> the fp64 library."""
    return L.load_f64() if dtype == torch.float64 else L.load()


def ptr(t: torch.Tensor) -> ctypes.c_void_p:
    return ctypes.c_void_p(t.data_ptr())


def stream_ptr(dev) -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


class DeviceState:
    """An accumulator whose arrays live in ``self._dev``, a tuple of device tensors that exists from the first update on; the fp64
    ones a record is made of come first.  Listed before the record class it completes."""

    _dev = None
    _shape = None
    _merge_into = "a host record"       # where a merge can go while this accumulator is still empty

    def _unset(self) -> bool:
        return self._dev is None

    def _read(self, count: int):
        """Host copies of the first ``count`` tensors."""
        if self._dev is None:
            raise RuntimeError("no sample recorded yet")
        return tuple(t.cpu().numpy() for t in self._dev[:count])

    def _write(self, *values) -> None:
        """``values`` into the first tensors."""
        if self._dev is None:
            raise RuntimeError(f"{type(self).__name__} takes a state only after its first update (merge into {self._merge_into} instead)")
        for t, v in zip(self._dev, values):
            t.copy_(torch.as_tensor(np.ascontiguousarray(v, np.float64)).reshape(t.shape))


class WallUnits:
    """Wall units of a record whose ``_state()[1]`` is ``mean [B, ny, K]`` with ``u`` as channel 0 (``VelocityStats``,
    ``TCF_tools.py:462-482, 1465-1478``): walls at ``y = -1`` and ``y = +1``."""

    y_centers = None                    # cell centres of the rows
    viscosity = None

    def set_wall_units(self, y_centers, viscosity: float):
        self.y_centers, self.viscosity = np.asarray(y_centers, np.float64).copy(), float(viscosity)
        return self

    def _need_wall(self):
        if self.y_centers is None or self.viscosity is None:
            raise RuntimeError("wall units need set_wall_units(y_centers, viscosity)")
        return self.y_centers, self.viscosity

    def u_wall(self) -> np.ndarray:
        """Friction velocity per env ``[B]`` from the mean-``u`` rows next to the two walls (``get_avg_u_wall``)."""
        y, nu = self._need_wall()
        u = self._state()[1][..., 0]
        if len(y) != u.shape[1]:
            raise RuntimeError("u_wall needs both walls: take it before half_channel()")
        return np.sqrt(0.5 * (u[:, 0] / (1.0 + y[0]) + u[:, -1] / (1.0 - y[-1])) * nu)
