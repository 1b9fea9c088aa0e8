"""RGB frames of the envs of a batch, on the GPU: the last step of the reference's ``_get_render_data`` /
``_format_render_data`` (``envs/fluid_env.py:710-747``) -- slice, flips, normalise, clip, 256-entry colour table, solid-body mask,
``uint8`` RGB -- as one kernel (``fg_frame_colorize``, ``csrc/fg_frames.hip``) over the views the envs already hold on the device,
and a recorder in the idiom of ``start_flow_statistics`` / ``stop_flow_statistics``.

``colorize`` is the door to the kernel, ``resolve_colormap`` the source of the colour tables, ``FrameRecording`` what
``FluidEnv.stop_frame_recording`` hands out.  The bytes are the ones
``sns.color_palette(name, as_cmap=True)(clip((d - vmin) / (vmax - vmin), 0, 1), bytes=True)[..., :3]`` gives for a float32 array.

Colour maps: ``viridis``, ``rainbow`` and ``coolwarm`` ship with the package (``colormaps.json``, sampled from matplotlib by
``tools/make_colormaps.py``; a text file, each table as hexadecimal digits, because the repository keeps binary files under
``tests/golden/`` only); any other name is looked up in seaborn, then matplotlib, when they import.  ``icefire`` -- the map of
the reference's vorticity pictures -- is seaborn's: without seaborn it falls back to ``coolwarm`` with one warning."""
from __future__ import annotations

import ctypes
import json
import os
import warnings
from dataclasses import dataclass
from pathlib import Path
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _lib as L

SHIPPED_COLORMAPS = ("viridis", "rainbow", "coolwarm")
_COLORMAPS_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "colormaps.json")
_shipped: Optional[Dict[str, np.ndarray]] = None
_resolved: Dict[str, np.ndarray] = {}
_icefire_warned = False


@dataclass(frozen=True)
class FrameSpec:
    """Which plane of a view ``[B, C, (z,) y, x]`` is drawn and how it is oriented; mirrors the C struct ``fg_frame_spec``.

    ``channel >= 0`` selects that channel, ``-1`` the Euclidean norm over all channels.  ``axis`` is ``-1`` for a 2-D view; ``0`` holds
    z fixed at ``index`` (rows y, columns x), ``1`` holds y fixed (rows z, columns x), ``2`` holds x fixed (rows z, columns y).  Then
    ``transpose``, then ``flip_rows`` / ``flip_cols`` of the transposed plane."""
    channel: int = 0
    axis: int = -1
    index: int = 0
    transpose: bool = False
    flip_rows: bool = False
    flip_cols: bool = False

    def c_struct(self) -> L.FgFrameSpec:
        return L.FgFrameSpec(int(self.channel), int(self.axis), int(self.index), int(bool(self.transpose)), int(bool(self.flip_rows)),
                             int(bool(self.flip_cols)))

    def frame_shape(self, nz: int, ny: int, nx: int) -> Tuple[int, int]:
        """``(H, W)`` of the frame this spec cuts from a field of ``nz x ny x nx`` cells."""
        rows, cols = {-1: (ny, nx), 0: (ny, nx), 1: (nz, nx), 2: (nz, ny)}[int(self.axis)]
        return (cols, rows) if self.transpose else (rows, cols)


def _load_shipped() -> Dict[str, np.ndarray]:
    global _shipped
    if _shipped is None:
        with open(_COLORMAPS_FILE) as f:          # a text file: name -> the table's 768 bytes as hexadecimal digits
            _shipped = {k: np.frombuffer(bytes.fromhex(v), dtype=np.uint8).reshape(256, 3).copy() for k, v in json.load(f).items()}
    return _shipped


def sample_colormap(cmap) -> np.ndarray:
    """The 256 RGB bytes a matplotlib colour map gives to the centres of 256 equal bins of [0, 1] -- for a 256-entry map, its table."""
    x = (np.arange(256, dtype=np.float64) + 0.5) / 256.0
    return np.ascontiguousarray(cmap(x, bytes=True)[:, :3].astype(np.uint8))


def _lookup_installed(name: str) -> Optional[np.ndarray]:
    try:
        import seaborn as sns
        return sample_colormap(sns.color_palette(name, as_cmap=True))
    except ImportError:
        pass
    except (ValueError, KeyError):      # seaborn is there and does not know the name: matplotlib may
        pass
    try:
        import matplotlib
        return sample_colormap(matplotlib.colormaps[name])
    except (ImportError, KeyError):
        return None


def resolve_colormap(name_or_table) -> np.ndarray:
    """``uint8 [256, 3]``: an array is checked (shape, dtype) and taken as is; ``viridis`` / ``rainbow`` / ``coolwarm`` come from the
    shipped file; any other name from seaborn, then matplotlib, when they import; ``icefire`` without seaborn is ``coolwarm`` with one
    warning; anything else is a ``ValueError`` naming the package that would know the map."""
    global _icefire_warned
    if not isinstance(name_or_table, str):
        table = name_or_table.detach().cpu().numpy() if isinstance(name_or_table, torch.Tensor) else np.asarray(name_or_table)
        if table.shape != (256, 3) or table.dtype != np.uint8:
            raise ValueError(f"a colour table must be uint8 [256, 3], got {table.dtype} {list(table.shape)}")
        return np.ascontiguousarray(table)
    name = name_or_table
    if name in SHIPPED_COLORMAPS:
        return _load_shipped()[name]
    if name in _resolved:
        return _resolved[name]
    table = _lookup_installed(name)
    if table is None and name == "icefire":
        if not _icefire_warned:
            warnings.warn("colour map 'icefire' is seaborn's and seaborn is not installed: using 'coolwarm' instead", RuntimeWarning,
                          stacklevel=2)
            _icefire_warned = True
        table = _load_shipped()["coolwarm"]      # kept under the name like any other: looked up once per process
    if table is None:
        raise ValueError(f"unknown colour map {name!r}: shipped are {SHIPPED_COLORMAPS}; other names need seaborn or matplotlib "
                         f"installed and knowing the map")
    _resolved[name] = table
    return table


def plane_values(view: torch.Tensor, spec: FrameSpec) -> torch.Tensor:
    """``[B, rows, cols]`` of the plane ``spec`` selects (before orientation), the norm formed as the kernel forms it:
    ``sqrt(((u0 u0) + (u1 u1)) + (u2 u2))``, every operation rounded on its own."""
    v = view if view.dim() == 5 else view.unsqueeze(2)
    if spec.axis in (-1, 0):
        v = v[:, :, spec.index]
    elif spec.axis == 1:
        v = v[:, :, :, spec.index]
    else:
        v = v[..., spec.index]
    if spec.channel >= 0:
        return v[:, spec.channel]
    s = v[:, 0] * v[:, 0]
    for k in range(1, v.shape[1]):
        s = s + v[:, k] * v[:, k]
    return torch.sqrt(s)


def range_over(values: torch.Tensor, symmetric: bool = False) -> torch.Tensor:
    """Float32 ``[B, 2]`` = ``(lo, span)`` per env from ``torch.aminmax`` over everything but axis 0 of ``values``; ``symmetric``:
    ``lo = -a``, ``hi = a``, ``a = max(|min|, |max|)``.  The span is the float32 difference; a NaN propagates."""
    v = values.detach().to(torch.float32)
    mn, mx = torch.aminmax(v.reshape(v.shape[0], -1), dim=1)
    if symmetric:
        a = torch.maximum(mn.abs(), mx.abs())
        mn, mx = -a, a
    return torch.stack([mn, mx - mn], dim=1)


def value_range_tensor(view: torch.Tensor, spec: FrameSpec, value_range, envs: torch.Tensor) -> torch.Tensor:
    """The kernel's ``range`` argument, float32 ``[n, 2]`` = ``(lo, span)`` per listed env, built on the device without a
    synchronisation.  ``(lo, hi)``: ``lo32 = float32(lo)``, ``span32 = float32(hi - lo)``, the difference taken in Python floats (as
    NumPy does with Python scalars).  ``"auto"``: per env ``torch.aminmax`` over the drawn plane -- or ``("auto", tensor)`` over a
    tensor ``[B, ...]`` the caller names --, the span the float32 difference; a NaN propagates (an all-black frame, as with
    ``np.min``).  ``"symmetric"`` / ``("symmetric", tensor)``: ``lo = -a``, ``hi = a``, ``a = max(|min|, |max|)``.  A float32 tensor
    ``[B, 2]`` is ``(lo, span)`` per env as it stands (``range_over``, taken once for several keys)."""
    B = view.shape[0]
    if isinstance(value_range, torch.Tensor):
        if tuple(value_range.shape) != (B, 2) or value_range.dtype != torch.float32:
            raise ValueError(f"a range tensor must be float32 [{B}, 2] = (lo, span) per env, got {value_range.dtype} {list(value_range.shape)}")
        return value_range.to(view.device).index_select(0, envs).contiguous()
    kind, over = value_range, None
    if isinstance(value_range, (tuple, list)) and len(value_range) == 2 and isinstance(value_range[0], str):
        kind, over = value_range
    if isinstance(kind, str):
        if kind not in ("auto", "symmetric"):
            raise ValueError(f"value_range must be (lo, hi), 'auto' or 'symmetric', got {kind!r}")
        over = plane_values(view, spec) if over is None else over
        if over.shape[0] != B:
            raise ValueError(f"the tensor a range is taken over needs one entry per env ({B}), got {over.shape[0]}")
        return range_over(over, kind == "symmetric").index_select(0, envs).contiguous()
    lo, hi = value_range
    n = envs.numel()          # two fills on the device: nothing is copied from the host
    return torch.stack([torch.full((n,), float(np.float32(lo)), dtype=torch.float32, device=view.device),
                        torch.full((n,), float(np.float32(float(hi) - float(lo))), dtype=torch.float32, device=view.device)], dim=1)


_env_indices: Dict[tuple, torch.Tensor] = {}


def env_index_tensor(env_list: np.ndarray, device) -> torch.Tensor:
    """The listed envs as an int64 index tensor on ``device``, uploaded once per distinct list and kept (a recording asks for the same
    list at every sample)."""
    device = torch.device(device)
    key = (device.type, device.index, env_list.tobytes())
    if key not in _env_indices:
        if len(_env_indices) >= 64:
            _env_indices.clear()
        _env_indices[key] = torch.from_numpy(env_list.astype(np.int64)).to(device)
    return _env_indices[key]


def colorize(view: torch.Tensor, spec: FrameSpec, table, value_range, mask=None, envs: Optional[Sequence[int]] = None) -> torch.Tensor:
    """``uint8 [n, H, W, 3]`` on the device of ``view``: the frames of the envs ``envs`` (default: all, in order; any order, repeats
    allowed) of the view ``[B, C, (z,) y, x]``.  ``table``: device ``uint8 [256, 3]`` (or anything ``resolve_colormap`` takes);
    ``value_range``: see ``value_range_tensor``; ``mask``: ``[H, W]`` in output orientation, non-zero / True marks a solid pixel.  One
    kernel launch per 64 listed envs, asynchronous on the current stream; there is no other path."""
    if not isinstance(view, torch.Tensor) or not view.is_cuda:
        raise L.NativeLibraryError("colorize needs a view on the GPU; fluidgym_amd has no CPU path")
    if view.dim() not in (4, 5):
        raise ValueError(f"a view is [B, C, (z,) y, x], got {list(view.shape)}")
    view = view.detach().to(torch.float32).contiguous()       # a single-block fp64 view is drawn through a cast
    B, C = int(view.shape[0]), int(view.shape[1])
    nz, ny, nx = ((1,) + tuple(int(s) for s in view.shape[2:]))[-3:]
    env_list = np.arange(B, dtype=np.int32) if envs is None else np.ascontiguousarray(np.asarray(envs, dtype=np.int64).reshape(-1)).astype(np.int32)
    if env_list.size == 0:
        raise ValueError("envs must list at least one env")
    if env_list.min() < 0 or env_list.max() >= B:
        raise ValueError(f"envs must lie in [0, {B}), got {env_list.tolist()}")
    if not isinstance(table, torch.Tensor) or not table.is_cuda:
        table = device_table(table, view.device)
    if table.dtype != torch.uint8 or tuple(table.shape) != (256, 3):
        raise ValueError(f"a colour table must be uint8 [256, 3], got {table.dtype} {list(table.shape)}")
    table = table.contiguous()
    H, W = spec.frame_shape(nz, ny, nx) if spec.axis in (-1, 0, 1, 2) else (1, 1)     # (an unknown axis is the library's to refuse)
    if mask is not None:
        if not (isinstance(mask, torch.Tensor) and mask.device == view.device and mask.dtype == torch.uint8):
            mask = torch.as_tensor(mask).to(device=view.device).ne(0).to(torch.uint8)
        mask = mask.contiguous()
        if tuple(mask.shape) != (H, W):
            raise ValueError(f"the mask must be [H, W] = [{H}, {W}] in output orientation, got {list(mask.shape)}")
    n = int(env_list.size)
    out = torch.empty((n, H, W, 3), dtype=torch.uint8, device=view.device)
    rng = value_range_tensor(view, spec, value_range, env_index_tensor(env_list, view.device))
    c_spec = spec.c_struct()
    stream = ctypes.c_void_p(torch.cuda.current_stream(view.device).cuda_stream)
    L.check(L.load().fg_frame_colorize(ctypes.c_void_p(view.data_ptr()), B, C, nz, ny, nx, ctypes.byref(c_spec),
                                       ctypes.c_void_p(table.data_ptr()), ctypes.c_void_p(mask.data_ptr()) if mask is not None else None,
                                       ctypes.c_void_p(rng.data_ptr()),
                                       env_list.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), n, ctypes.c_void_p(out.data_ptr()), stream))
    return out


_device_tables: Dict[tuple, torch.Tensor] = {}


def device_table(name_or_table, device) -> torch.Tensor:
    """The colour table on ``device``; a named map (the ``icefire`` fallback included) is uploaded once per device and kept."""
    device = torch.device(device)
    if isinstance(name_or_table, str):
        key = (name_or_table, device.type, device.index)
        if key not in _device_tables:
            _device_tables[key] = torch.from_numpy(resolve_colormap(name_or_table)).to(device)
        return _device_tables[key]
    return torch.from_numpy(resolve_colormap(name_or_table)).to(device)


# ---- the planes of the reference's _get_render_data per env family, net of its flips (it flips the field, _format_render_data flips
# the columns again).  Its indices are taken as its lines write them: in 3-D its vorticity is [3, z, y, x], so ``vorticity.shape[0] // 2``
# is 3 // 2 = 1, ``shape[1]`` is nz and ``shape[2]`` is ny, while its temperature and speed are [z, y, x] and their ``shape[0] // 2`` etc.
# are the mid planes.  An index outside its axis is refused by the library, as the reference's slice raises.
def rbc_frame_specs(ndims: int, shape) -> Dict[str, FrameSpec]:
    """rbc_env_base.py:541-577 for a temperature ``[(z,) y, x]`` of extents ``shape``: 2-D and x-y (mid z) rows and columns flipped,
    x-z (mid y) columns flipped, y-z (mid x) the columns of ``[z, y]`` flipped and then the transpose."""
    if ndims == 2:
        return {"temperature": FrameSpec(0, -1, 0, flip_rows=True, flip_cols=True)}
    nz, ny, nx = (int(v) for v in shape)
    return {"x-y-temperature": FrameSpec(0, 0, nz // 2, flip_rows=True, flip_cols=True),
            "x-z-temperature": FrameSpec(0, 1, ny // 2, flip_cols=True),
            "y-z-temperature": FrameSpec(0, 2, nx // 2, transpose=True, flip_rows=True)}


def vortex_frame_specs(ndims: int, shape, flip_y: bool) -> Dict[str, FrameSpec]:
    """cylinder_env_base.py:700-739 (``flip_y`` False: the field's x is flipped) and airfoil_env_base.py:664-702 (``flip_y`` True: y
    and x are) for a vorticity ``[1, y, x]`` / ``[3, z, y, x]``.  3-D, on the flipped ``[3, z, y, x]`` array: component 2 at z index
    ``shape[0] // 2 = 1``; component 1 at y index ``shape[1] // 2 = nz // 2``; component 0 at x index ``int(shape[2] * 0.8) =
    int(ny * 0.8)``, as ``[z, y]`` transposed, whose columns (z) the formatting then flips."""
    if ndims == 2:
        return {"vorticity": FrameSpec(0, -1, 0, flip_rows=flip_y)}
    nz, ny, nx = (int(v) for v in shape)
    y_index, x_index = nz // 2, int(ny * 0.8)                # of the flipped field
    return {"x-y-vorticity": FrameSpec(2, 0, 3 // 2, flip_rows=flip_y),
            "x-z-vorticity": FrameSpec(1, 1, ny - 1 - y_index if flip_y else y_index),
            "y-z-vorticity": FrameSpec(0, 2, nx - 1 - x_index, transpose=True, flip_rows=flip_y, flip_cols=True)}


def tcf_frame_specs(shape, wall_row: int) -> Dict[str, FrameSpec]:
    """tcf_env.py:679-751 for fields of ``nz x ny x nx`` cells, y and x flipped by the reference; ``wall_row`` is the (unflipped) row
    of the wall-parallel pictures.  Speed ``[z, y, x]`` (:735-737): mid z, the wall row, mid x of the flipped field.  Vorticity
    ``[3, z, y, x]`` (:745-747): component 2 at z index ``shape[0] // 2 = 1``, component 1 at the wall row, component 0 at x index
    ``shape[2] // 2 = ny // 2`` of the flipped field.  Net: y flipped, x not, the z columns of the transposed y-z planes flipped."""
    nz, ny, nx = (int(v) for v in shape)
    yz = dict(axis=2, transpose=True, flip_rows=True, flip_cols=True)
    return {"x-y-velocity": FrameSpec(-1, 0, nz // 2, flip_rows=True),
            "x-z-velocity": FrameSpec(-1, 1, int(wall_row)),
            "y-z-velocity": FrameSpec(-1, index=nx - 1 - nx // 2, **yz),
            "x-y-vorticity": FrameSpec(2, 0, 3 // 2, flip_rows=True),
            "x-z-vorticity": FrameSpec(1, 1, int(wall_row)),
            "y-z-vorticity": FrameSpec(0, index=nx - 1 - ny // 2, **yz)}


class FrameRecording:
    """What ``FluidEnv.stop_frame_recording`` hands out: ``frames[key]`` is ``uint8 [T, n, H, W, 3]`` on the host, ``envs`` the
    recorded envs in the order of axis 1, ``steps`` the env-step counter of every sample (0 = the sample taken at the start)."""

    def __init__(self, frames: Dict[str, np.ndarray], envs: Sequence[int], steps: Sequence[int], fps: int = 24):
        self.frames = {k: np.asarray(v) for k, v in frames.items()}
        self.envs = [int(e) for e in envs]
        self.steps = [int(s) for s in steps]
        self.fps = int(fps)
        for k, v in self.frames.items():
            if v.dtype != np.uint8 or v.ndim != 5 or v.shape[-1] != 3 or v.shape[0] != len(self.steps) or v.shape[1] != len(self.envs):
                raise ValueError(f"frames[{k!r}] must be uint8 [T={len(self.steps)}, n={len(self.envs)}, H, W, 3], got {v.dtype} {list(v.shape)}")

    def __len__(self) -> int:
        return len(self.steps)

    def _column(self, env: int) -> int:
        if int(env) not in self.envs:
            raise ValueError(f"env {env} was not recorded (recorded: {self.envs})")
        return self.envs.index(int(env))

    def save_png(self, output_path, env: int, t: int = -1) -> Dict[str, Path]:
        """One ``<key>_env<env>_<step>.png`` per key: sample ``t`` of env ``env``.  Returns key -> path."""
        from PIL import Image

        out_dir = Path(output_path)
        out_dir.mkdir(parents=True, exist_ok=True)
        col, written = self._column(env), {}
        for key, v in self.frames.items():
            path = out_dir / f"{key}_env{int(env)}_{self.steps[t]:06d}.png"
            Image.fromarray(np.ascontiguousarray(v[t, col])).save(path)
            written[key] = path
        return written

    def save_gif(self, filename: str, output_path=None, env: Optional[int] = None) -> Dict[Tuple[str, int], Path]:
        """One GIF per key and recorded env (or the env ``env`` alone), ``<key>_<filename>.gif`` as the reference names them
        (``fluid_env.py:993-1018``) -- with more than one env written, ``<key>_env<e>_<filename>.gif`` --, ``1000 / render_fps`` ms per
        frame, looping.  Every sample is written: the reference's thinning to 500 frames is not copied.  Returns (key, env) -> path."""
        from PIL import Image

        out_dir = Path("." if output_path is None else output_path)
        out_dir.mkdir(parents=True, exist_ok=True)
        stem = filename[:-4] if filename.endswith(".gif") else filename
        chosen = self.envs if env is None else [int(env)]
        if len(self) == 0:
            raise ValueError("save_gif: the recording holds no sample")
        written = {}
        for key, v in self.frames.items():
            for e in dict.fromkeys(chosen):
                col = self._column(e)
                name = f"{key}_{stem}.gif" if len(set(chosen)) == 1 else f"{key}_env{e}_{stem}.gif"
                images = [Image.fromarray(np.ascontiguousarray(v[t, col])) for t in range(len(self))]
                images[0].save(out_dir / name, save_all=True, append_images=images[1:], duration=1000.0 / self.fps, loop=0)
                written[(key, e)] = out_dir / name
        return written


class FrameRecorder:
    """The device-to-host side of a recording: every sample is copied into pinned memory asynchronously, behind the kernel on the
    stream that drew it; ``finish`` waits once and stacks."""

    def __init__(self, envs: Sequence[int], every: int, fps: int, size_3d: Optional[Tuple[int, int]] = None):
        """``size_3d``: ``(H, W)`` of the 3-D keys a recording with ``render_3d=True`` adds to every sample, or None."""
        self.envs = [int(e) for e in envs]
        self.size_3d = None if size_3d is None else (int(size_3d[0]), int(size_3d[1]))
        self.every, self.tick, self.fps = int(every), 0, int(fps)
        self.steps: list = []
        self.samples: Dict[str, list] = {}

    def add(self, frames: Dict[str, torch.Tensor], step: int) -> None:
        for key, t in frames.items():
            host = torch.empty(t.shape, dtype=torch.uint8, pin_memory=True)
            host.copy_(t, non_blocking=True)
            self.samples.setdefault(key, []).append(host)
        self.steps.append(int(step))

    def finish(self) -> FrameRecording:
        torch.cuda.synchronize()
        frames = {k: np.stack([h.numpy() for h in v]) for k, v in self.samples.items()}
        return FrameRecording(frames, self.envs, self.steps, self.fps)
