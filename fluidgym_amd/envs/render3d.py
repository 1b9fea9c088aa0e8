"""3-D frames of the envs of a batch, on the GPU: the reference's ``render(render_3d=True)`` -- marching cubes
plus a matplotlib ``Poly3DCollection`` (``envs/util/visualization.py:211-379``) and ``ax.voxels`` (``:382-475``) -- as one ray marcher
(``fg_render_isosurface`` / ``fg_render_volume``, ``csrc/fg_render3d.hip``) over the volumes the envs already hold on the device.

``orbit_camera`` builds the camera, ``raycast_isosurface`` and ``raycast_volume`` are the doors to the kernel, ``log_opacity_table``
the reference's voxel opacity as a per-step table.  ``FluidEnv.render_frames_3d`` feeds them with the per-family specs.

Camera convention (derived from what the reference's call does: ``transpose(0, 2, 1)`` puts the simulation's y on matplotlib's
vertical axis and its z on matplotlib's y axis, ``invert_xaxis`` -- kept by ``set_xlim(hi, lo)`` -- turns the x axis round, the
``invert_yaxis`` is undone by ``set_ylim(lo, hi)``; ``view_init(elev, azim)`` then puts the viewer at ``(cos e cos a, cos e sin a,
sin e)`` of the box as displayed).  In simulation axes ``(x, y, z)``, with ``up_axis="y"``, the viewer stands in the direction

    ``v = (-cos(elev) cos(azim), sin(elev), cos(elev) sin(azim))``

from the centre of the box and looks at the centre; y points up in the image.  So at ``azim = 0`` the low-x (inflow) face is the
nearest and +z points to the right of the image; at ``azim = 90`` the high-z face is nearest and +x points right; at 180 the high-x
face, -z right; at 270 the low-z face, -x right; a positive ``elev`` looks down on the top (high-y) face.  The default views
(``azim`` 45 or 60) therefore show the inflow face and the high-z side, the flow running from the near left to the far right.  The
image is never mirrored (the camera frame is right-handed: right = forward x up).  The reference's voxel picture of ``RBC3D`` passes its
``[z, y, x]`` array as ``(X, Y, Z)`` and keeps both axes inverted, which is a mirror image of a box that is square and periodic in x
and z; it is drawn here by the same convention as the surfaces.  ``up_axis`` "z" / "x" permute the roles: the horizontal axes are then
``(y, x)`` / ``(z, y)`` in place of ``(x, z)``."""
from __future__ import annotations

import ctypes
import math
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _lib as L
from . import frames as F

AMBIENT, DIFFUSE = 0.35, 0.65            # the headlight: ambient + diffuse |n.d| / (|n| |d|)
BODY_COLOR = (128, 128, 128)             # the reference draws its cylinder and airfoil in "gray"
_AXES = {"x": 0, "y": 1, "z": 2}
_HORIZONTAL = {"y": (0, 2), "z": (1, 0), "x": (2, 1)}      # (h1, h2): the viewer stands at -cos a h1 + sin a h2 (times cos e) + sin e up


class Camera(L.FgRenderCamera):
    """``fg_render_camera`` (the six vectors, passed to the library as they stand) with the image it was built for: ``size = (H, W)``,
    or None for a camera made of vectors by hand, whose image size the doors then ask for.  ``copy.copy`` keeps both."""
    size: Optional[Tuple[int, int]] = None


def camera_from_vectors(o0, ou, ov, d0, du, dv, size=None) -> Camera:
    """The camera struct from six vectors ``(x, y, z)`` of index space (rounded to float32 here, once)."""
    cam = Camera()
    cam.size = None if size is None else (int(size[0]), int(size[1]))
    for name, vec in zip(("o0", "ou", "ov", "d0", "du", "dv"), (o0, ou, ov, d0, du, dv)):
        v = np.asarray(vec, dtype=np.float64).reshape(3)
        setattr(cam, name, (ctypes.c_float * 3)(*[float(np.float32(x)) for x in v]))
    return cam


def camera_array(camera: L.FgRenderCamera) -> np.ndarray:
    """The 18 float32 entries of a camera, ``[6, 3]`` in the order ``o0, ou, ov, d0, du, dv``."""
    return np.array([list(getattr(camera, name)) for name in ("o0", "ou", "ov", "d0", "du", "dv")], dtype=np.float32)


def orbit_camera(shape, extent, elev: float, azim: float, size=(480, 640), projection: str = "persp", up_axis: str = "y",
                 zoom: float = 1.0) -> Camera:
    """The camera that looks at the centre of a box of ``shape = (nz, ny, nx)`` samples and physical size ``extent = (Lx, Ly, Lz)``
    from the direction ``elev`` / ``azim`` (degrees) name (the module docstring holds the convention), for an image of
    ``size = (H, W)`` square pixels.  The bounding sphere of the box fills the smaller image dimension at ``zoom = 1``.  ``"ortho"``:
    parallel rays (``du = dv = 0``); ``"persp"``: all rays from one eye (``ou = ov = 0``) four sphere radii from the centre; both
    start on the same plane, share the ray through the image centre, and ``t`` counts physical length along the central direction.
    Trigonometry in float64 on the host; the world -> index mapping ``index_a = (w_a / L_a + 1/2) (n_a - 1)`` is folded in."""
    if projection not in ("persp", "ortho"):
        raise ValueError(f"projection must be 'persp' or 'ortho', got {projection!r}")
    if up_axis not in _AXES:
        raise ValueError(f"up_axis must be 'x', 'y' or 'z', got {up_axis!r}")
    H, W = (int(s) for s in size)
    if H < 1 or W < 1:
        raise ValueError(f"size must be (H, W) with H, W >= 1, got {tuple(size)}")
    nz, ny, nx = (int(s) for s in shape)
    if min(nz, ny, nx) < 2:
        raise ValueError(f"every extent of the volume must be at least 2, got shape {tuple(shape)}")
    ext = np.asarray(extent, dtype=np.float64).reshape(-1)
    if ext.shape != (3,) or not np.all(np.isfinite(ext)) or np.any(ext <= 0):
        raise ValueError(f"extent must be three positive physical sizes (Lx, Ly, Lz), got {extent}")
    if not (zoom > 0 and math.isfinite(zoom)):
        raise ValueError(f"zoom must be positive, got {zoom}")
    e, a = math.radians(float(elev)), math.radians(float(azim))
    h1, h2 = _HORIZONTAL[up_axis]
    up = np.zeros(3)
    up[_AXES[up_axis]] = 1.0
    v = math.sin(e) * up
    v[h1] += -math.cos(e) * math.cos(a)
    v[h2] += math.cos(e) * math.sin(a)
    f = -v                                                    # forward: from the viewer to the centre
    right = np.cross(f, up)
    if np.linalg.norm(right) < 1e-12:                         # looking straight down or up: the azimuth still names the right
        right = np.zeros(3)
        right[h1] += math.sin(a)
        right[h2] += math.cos(a)
    right /= np.linalg.norm(right)
    true_up = np.cross(right, f)
    radius = 0.5 * float(np.linalg.norm(ext))
    pixel = 2.0 * radius / (zoom * min(H, W))
    dist = 4.0 * radius
    scale = (np.array([nx, ny, nz], dtype=np.float64) - 1.0) / ext        # world -> index, per axis
    centre = 0.5 * (np.array([nx, ny, nz], dtype=np.float64) - 1.0)
    # the image plane through the eye: pixel (i, j) sits at eye + (j + 1/2 - W/2) pixel right + (H/2 - (i + 1/2)) pixel up
    eye = centre + dist * v * scale
    corner = (-0.5 * W * pixel) * right + (0.5 * H * pixel) * true_up
    col, row = pixel * right, -pixel * true_up
    zero = np.zeros(3)
    if projection == "ortho":
        return camera_from_vectors(eye + corner * scale, col * scale, row * scale, f * scale, zero, zero, size=(H, W))
    # a ray through the same point of the plane at the centre's depth: direction f + offset / dist
    return camera_from_vectors(eye, zero, zero, (f + corner / dist) * scale, col / dist * scale, row / dist * scale, size=(H, W))


def default_step(camera: L.FgRenderCamera) -> float:
    """Half a cell along the direction ``d`` of the ray through the image centre (``d0`` itself for a camera without a size):
    ``0.5 / |d|``, ``d`` in index space."""
    c = camera_array(camera).astype(np.float64)
    H, W = getattr(camera, "size", None) or (0, 0)
    d = c[3] + 0.5 * W * c[4] + 0.5 * H * c[5]
    return float(np.float32(0.5 / np.linalg.norm(d)))


def log_opacity_table(strength: float = 0.05) -> np.ndarray:
    """Float32 ``[256]``: the opacity one step adds to a sample that falls into bin ``k`` of the colour table.  The reference's voxels
    carry ``alpha = log1p(x) / max log1p(x)`` of the normalised value ``x`` (``visualization.py:437-441``, the maximum taken as
    ``log 2``, the value at ``x = 1``); a voxel there is one cell thick, a sample here is ``step`` thick, so ``strength`` is the
    opacity of one step through the hottest value: ``opacity[k] = strength log1p((k + 1/2) / 256) / log 2``.  Halving the step
    length asks for ``1 - sqrt(1 - strength)``, about half the strength, to keep the picture."""
    if not 0.0 <= float(strength) <= 1.0:
        raise ValueError(f"strength must lie in [0, 1], got {strength}")
    x = (np.arange(256, dtype=np.float64) + 0.5) / 256.0
    return (float(strength) * np.log1p(x) / math.log(2.0)).astype(np.float32)


_device_floats: Dict[tuple, torch.Tensor] = {}


def device_floats(values, device) -> torch.Tensor:
    """Host numbers as a float32 tensor on ``device``, uploaded once per distinct content and kept, as ``frames.device_table`` keeps the
    colour tables (an opacity table, or one level per env, is the same at every sample of a recording)."""
    device = torch.device(device)
    host = np.ascontiguousarray(np.asarray(values, dtype=np.float32))
    key = (device.type, device.index, host.shape, host.tobytes())
    if key not in _device_floats:
        if len(_device_floats) >= 64:
            _device_floats.clear()
        _device_floats[key] = torch.from_numpy(host.copy()).to(device)
    return _device_floats[key]


def _common(view: torch.Tensor, who: str, envs):
    if not isinstance(view, torch.Tensor) or not view.is_cuda:
        raise L.NativeLibraryError(f"{who} needs a view on the GPU; fluidgym_amd has no CPU path")
    if view.dim() != 5:
        raise ValueError(f"a volume view is [B, C, z, y, x], got {list(view.shape)}")
    view = view.detach().to(torch.float32).contiguous()       # a single-block fp64 view is drawn through a cast
    B = int(view.shape[0])
    env_list = np.arange(B, dtype=np.int32) if envs is None else np.ascontiguousarray(np.asarray(envs, dtype=np.int64).reshape(-1)).astype(np.int32)
    if env_list.size == 0:
        raise ValueError("envs must list at least one env")
    if env_list.min() < 0 or env_list.max() >= B:
        raise ValueError(f"envs must lie in [0, {B}), got {env_list.tolist()}")
    return view, env_list


def _table(table, device) -> torch.Tensor:
    if not isinstance(table, torch.Tensor) or not table.is_cuda:
        table = F.device_table(table, device)
    if table.dtype != torch.uint8 or tuple(table.shape) != (256, 3):
        raise ValueError(f"a colour table must be uint8 [256, 3], got {table.dtype} {list(table.shape)}")
    return table.contiguous()


def _options(step, camera, clip, body_color, background, ambient=AMBIENT, diffuse=DIFFUSE) -> L.FgRenderOptions:
    opt = L.FgRenderOptions()
    opt.step = default_step(camera) if step is None else float(step)
    opt.ambient, opt.diffuse = float(ambient), float(diffuse)
    opt.has_clip = 0 if clip is None else 1
    if clip is not None:
        lo, hi = clip
        opt.clip_lo = (ctypes.c_float * 3)(*[float(x) for x in lo])
        opt.clip_hi = (ctypes.c_float * 3)(*[float(x) for x in hi])
    opt.body_color = (ctypes.c_uint8 * 4)(*[int(c) for c in body_color], 0)
    opt.background = (ctypes.c_uint8 * 4)(*[int(c) for c in background], 0)
    return opt


def _range(view: torch.Tensor, channel: int, value_range, env_index: torch.Tensor) -> torch.Tensor:
    """``(lo, span)`` per listed env (``frames.value_range_tensor``); ``"auto"`` is taken over the whole drawn scalar of the volume."""
    if isinstance(value_range, str):
        scalar = view[:, channel] if channel >= 0 else _norm(view)
        value_range = (value_range, scalar)
    return F.value_range_tensor(view, F.FrameSpec(channel=channel, axis=0), value_range, env_index)


def _norm(view: torch.Tensor) -> torch.Tensor:
    s = view[:, 0] * view[:, 0]
    for k in range(1, view.shape[1]):
        s = s + view[:, k] * view[:, k]
    return torch.sqrt(s)


def raycast_isosurface(view: torch.Tensor, channel: int, level, color_view: torch.Tensor, color_channel: int, color_range, table,
                       camera: L.FgRenderCamera, clip=None, solid=None, body_color=BODY_COLOR, background=(255, 255, 255),
                       envs: Optional[Sequence[int]] = None, return_depth: bool = False, size=None, step: Optional[float] = None):
    """``uint8 [n, H, W, 3]`` on the device of ``view``: the surface ``|f| = level`` of the envs ``envs`` (default: all, in order; any
    order, repeats allowed) of the view ``[B, C, z, y, x]``, seen through ``camera`` in an image of ``size = (H, W)`` (default: the size ``orbit_camera`` built the camera for).  ``channel >= 0``
    selects that channel, ``-1`` the norm; ``level``: a number, or one per env of the batch (``[B]``; a device tensor, or host numbers that are uploaded once and kept); ``color_view`` / ``color_channel``
    / ``color_range`` (see ``frames.value_range_tensor``; ``"auto"`` over the whole volume) / ``table`` colour the surface; ``clip =
    ((x0, y0, z0), (x1, y1, z1))`` in index space bounds the surface; ``solid``: ``[z, y, x]``, non-zero inside a body shared by the
    envs, drawn in ``body_color``.  ``step``: the distance between samples in ``t`` (default: half a cell along the central ray).
    ``return_depth=True`` adds float32 ``[n, H, W]``, ``t`` of the hit or ``+inf``.  One launch per 64 listed envs, asynchronous on
    the current stream; there is no other path."""
    view, env_list = _common(view, "raycast_isosurface", envs)
    size = getattr(camera, "size", None) if size is None else size
    if size is None:
        raise ValueError("size=(H, W) is required for a camera that orbit_camera did not build")
    H, W = (int(s) for s in size)
    B, C, nz, ny, nx = (int(s) for s in view.shape)
    if not isinstance(color_view, torch.Tensor) or color_view.device != view.device or tuple(color_view.shape[2:]) != (nz, ny, nx) \
            or color_view.dim() != 5 or int(color_view.shape[0]) != B:
        raise ValueError(f"color_view must be [B, C', z, y, x] on the view's device with the view's extents {[B, nz, ny, nx]}")
    color_view = color_view.detach().to(torch.float32).contiguous()
    table = _table(table, view.device)
    env_index = F.env_index_tensor(env_list, view.device)
    if isinstance(level, torch.Tensor):
        lev = level.detach().to(device=view.device, dtype=torch.float32).reshape(-1)
    elif np.ndim(level) == 0:         # one number: a fill on the device, nothing is copied from the host
        lev = torch.full((B,), float(np.float32(level)), dtype=torch.float32, device=view.device)
    else:
        lev = device_floats(np.asarray(level, dtype=np.float32).reshape(-1), view.device)
    if lev.numel() == 1:
        lev = lev.expand(B)
    if lev.numel() != B:
        raise ValueError(f"level must be one number or one per env ({B}), got {lev.numel()}")
    lev = lev.index_select(0, env_index).contiguous()
    rng = _range(color_view, int(color_channel), color_range, env_index)
    if solid is not None:
        if not (isinstance(solid, torch.Tensor) and solid.device == view.device and solid.dtype == torch.uint8):
            solid = torch.as_tensor(np.asarray(solid)).to(device=view.device).ne(0).to(torch.uint8)
        solid = solid.contiguous()
        if tuple(solid.shape) != (nz, ny, nx):
            raise ValueError(f"the solid mask must be [z, y, x] = {[nz, ny, nx]}, got {list(solid.shape)}")
    opt = _options(step, camera, clip, body_color, background)
    n = int(env_list.size)
    out = torch.empty((n, max(H, 0), max(W, 0), 3), dtype=torch.uint8, device=view.device)
    depth = torch.empty((n, max(H, 0), max(W, 0)), dtype=torch.float32, device=view.device) if return_depth else None
    stream = ctypes.c_void_p(torch.cuda.current_stream(view.device).cuda_stream)
    L.check(L.load().fg_render_isosurface(
        ctypes.c_void_p(view.data_ptr()), B, C, nz, ny, nx, int(channel), ctypes.c_void_p(lev.data_ptr()),
        ctypes.c_void_p(color_view.data_ptr()), int(color_view.shape[1]), int(color_channel), ctypes.c_void_p(rng.data_ptr()),
        ctypes.c_void_p(table.data_ptr()), ctypes.c_void_p(solid.data_ptr()) if solid is not None else None, ctypes.byref(camera),
        ctypes.byref(opt), H, W, env_list.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), n, ctypes.c_void_p(out.data_ptr()),
        ctypes.c_void_p(depth.data_ptr()) if depth is not None else None, stream))
    return (out, depth) if return_depth else out


def raycast_volume(view: torch.Tensor, channel: int, value_range, table, opacity, camera: L.FgRenderCamera,
                   background=(255, 255, 255), envs: Optional[Sequence[int]] = None, size=None, step: Optional[float] = None) -> torch.Tensor:
    """``uint8 [n, H, W, 3]`` on the device of ``view``: the emission-absorption picture of the scalar (``channel >= 0``, or ``-1``:
    the norm) of the view ``[B, C, z, y, x]``: every sample falls into a bin of ``table`` by ``value_range``, adds that colour with the
    per-step opacity ``opacity[bin]`` (float32 ``[256]``, e.g. ``log_opacity_table``; a host table is uploaded once per device and kept) front to back, and what is left shows the
    ``background``.  One launch per 64 listed envs, asynchronous on the current stream; there is no other path."""
    view, env_list = _common(view, "raycast_volume", envs)
    size = getattr(camera, "size", None) if size is None else size
    if size is None:
        raise ValueError("size=(H, W) is required for a camera that orbit_camera did not build")
    H, W = (int(s) for s in size)
    B, C, nz, ny, nx = (int(s) for s in view.shape)
    table = _table(table, view.device)
    if not isinstance(opacity, torch.Tensor):
        opacity = device_floats(opacity, view.device)
    opacity = opacity.detach().to(device=view.device, dtype=torch.float32).contiguous()
    if tuple(opacity.shape) != (256,):
        raise ValueError(f"the opacity table must be float32 [256], got {list(opacity.shape)}")
    rng = _range(view, int(channel), value_range, F.env_index_tensor(env_list, view.device))
    opt = _options(step, camera, None, BODY_COLOR, background)
    n = int(env_list.size)
    out = torch.empty((n, max(H, 0), max(W, 0), 3), dtype=torch.uint8, device=view.device)
    stream = ctypes.c_void_p(torch.cuda.current_stream(view.device).cuda_stream)
    L.check(L.load().fg_render_volume(
        ctypes.c_void_p(view.data_ptr()), B, C, nz, ny, nx, int(channel), ctypes.c_void_p(rng.data_ptr()), ctypes.c_void_p(table.data_ptr()),
        ctypes.c_void_p(opacity.data_ptr()), ctypes.byref(camera), ctypes.byref(opt), H, W,
        env_list.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), n, ctypes.c_void_p(out.data_ptr()), stream))
    return out
