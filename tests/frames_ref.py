"""NumPy restatement of the frames, the checker of ``tests/test_frames_host.py`` and ``tests/test_gpu_frames.py``.

Two layers, written independently of ``fluidgym_amd/envs/frames.py``:
- ``colorize``: ``fg_frame_colorize`` step by step -- slice, transpose, flips, norm, normalise, clip, index, mask -- in float32 with
  every operation rounded on its own;
- the per-family recipes, written the way the reference's ``_get_render_data`` writes them (flip the field, slice with ITS index
  expressions -- ``shape[0] // 2`` of the ``[3, z, y, x]`` vorticity is 1, not the mid plane --, format -- which flips the columns --,
  flip or transpose the picture), NOT through a folded spec: they check the planes and orientations the envs state.
Byte equality is the contract everywhere."""
import numpy as np


def lookup(x, table):
    """``cmap(x, bytes=True)[..., :3]`` of a 256-entry map for float32 ``x`` already clipped to [0, 1] (NaN allowed): NaN is
    (0, 0, 0), else ``table[min(int(x * 256), 255)]``."""
    x = np.asarray(x, np.float32)
    nan = np.isnan(x)
    with np.errstate(invalid="ignore"):
        idx = np.minimum((np.where(nan, np.float32(0), x) * np.float32(256)).astype(np.int64), 255)
    rgb = np.asarray(table, np.uint8)[idx]
    rgb[nan] = 0
    return rgb


def normalise(d, lo, span):
    """``clip((d - lo) / span, 0, 1)`` in float32 (``lo``, ``span`` float32 scalars); NaN stays NaN."""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        x = (np.asarray(d, np.float32) - np.float32(lo)) / np.float32(span)
        return np.clip(x, np.float32(0), np.float32(1))


def fixed_range(lo, hi):
    """``(lo32, span32)`` of a range given as Python numbers: the difference is taken in Python floats."""
    return np.float32(lo), np.float32(float(hi) - float(lo))


def auto_range(values, symmetric=False):
    """``(lo32, span32)`` from the float32 array ``values``; NaN propagates."""
    v = np.asarray(values, np.float32)
    mn, mx = np.min(v), np.max(v)
    if symmetric:
        a = np.maximum(np.abs(mn), np.abs(mx))
        mn, mx = -a, a
    with np.errstate(invalid="ignore", over="ignore"):
        return np.float32(mn), np.float32(mx - mn)


def norm(field):
    """``sqrt(((u0 u0) + (u1 u1)) + (u2 u2))`` over axis 0, float32, each operation rounded on its own."""
    f = np.asarray(field, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        s = f[0] * f[0]
        for k in range(1, f.shape[0]):
            s = s + f[k] * f[k]
        return np.sqrt(s)


def plane(field, channel, axis, index):
    """The plane ``[rows, cols]`` of one env's field ``[C, nz, ny, nx]`` before orientation."""
    f = np.asarray(field, np.float32)
    sl = {-1: np.s_[:, index], 0: np.s_[:, index], 1: np.s_[:, :, index], 2: np.s_[:, :, :, index]}[axis]
    p = f[sl]
    return norm(p) if channel < 0 else p[channel]


def colorize(field, channel, axis, index, transpose, flip_rows, flip_cols, table, lo_span, mask=None, envs=None):
    """``fg_frame_colorize``: ``field [B, C, nz, ny, nx]`` float32, ``lo_span [n, 2]`` per listed env -> ``uint8 [n, H, W, 3]``."""
    field = np.asarray(field, np.float32)
    envs = list(range(field.shape[0])) if envs is None else list(envs)
    out = []
    for i, e in enumerate(envs):
        p = plane(field[e], channel, axis, index)
        if transpose:
            p = p.T
        if flip_rows:
            p = p[::-1]
        if flip_cols:
            p = p[:, ::-1]
        rgb = lookup(normalise(p, lo_span[i][0], lo_span[i][1]), table)
        if mask is not None:
            rgb[np.asarray(mask) != 0] = 0
        out.append(rgb)
    return np.stack(out)


# ---- the reference's own sequence of steps (envs/fluid_env.py:741-747) and the recipes built on it ---------------------------------
def format_render_data(data, lo, span, table):
    """``_format_render_data``: flip the columns, normalise, clip, colour."""
    return lookup(normalise(np.flip(np.asarray(data, np.float32), axis=1), lo, span), table)


def channel_frames(u, table):
    """The channel envs of this project: the speed in its own range, no flips; mid z in 3-D.  ``u [d, (z,) y, x]`` of one env."""
    speed = norm(u)
    if speed.ndim == 3:
        speed = speed[speed.shape[0] // 2]
    lo, span = auto_range(speed)
    return {"velocity": lookup(normalise(speed, lo, span), table)}


def rbc_frames(T, T_cold, T_max, table):
    """rbc_env_base.py:541-577 with the range ``(T_cold, T_max)`` applied in one step.  ``T [(z,) y, x]`` of one env."""
    lo, span = fixed_range(T_cold, T_max)
    fmt = lambda d: format_render_data(d, lo, span, table)
    if T.ndim == 2:
        return {"temperature": np.flipud(fmt(T))}
    return {
        "x-y-temperature": np.flipud(fmt(T[T.shape[0] // 2, :, :])),
        "x-z-temperature": fmt(T[:, T.shape[1] // 2, :]),
        "y-z-temperature": fmt(T[:, :, T.shape[2] // 2]).transpose(1, 0, 2),
    }


def cylinder_mask(render_shape, ndims, H=4.1, L=22.0, diameter=1.0):
    """cylinder_env_base.py:518-535."""
    radius = diameter / 2 * (render_shape[1] - 1) / H
    cx = round((render_shape[0] - 1) / L * 2.0)
    cy = round((render_shape[1] - 1) / H * 2.0)
    Y, X = np.ogrid[: render_shape[1], : render_shape[0]]
    m = np.sqrt((X - cx) ** 2 + (Y - cy) ** 2) <= radius
    return np.repeat(m[None], render_shape[2], axis=0) if ndims == 3 else m


def _vortex_frames(w, flip_axes, lo, span, table, mask):
    """The body cylinder_env_base.py:700-739 and airfoil_env_base.py:664-702 share.  ``w [1, y, x]`` or ``[3, z, y, x]`` of one env."""
    w = np.asarray(w, np.float32)
    w = np.flip(w[0] if w.ndim == 3 else w, axis=flip_axes)
    fmt = lambda d: format_render_data(d, lo, span, table)
    out = {}
    if w.ndim == 2:
        out["vorticity"] = fmt(w)
        if mask is not None:
            out["vorticity"][mask] = 0
        return out
    # the reference's own indices on its [3, z, y, x] array: shape[0] is 3 (so z plane 1), shape[1] is nz, shape[2] is ny
    out["x-y-vorticity"] = fmt(w[2, w.shape[0] // 2, :, :])
    out["x-z-vorticity"] = fmt(w[1, :, w.shape[1] // 2, :])
    out["y-z-vorticity"] = fmt(w[0, :, :, int(w.shape[2] * 0.8)].T)
    if mask is not None:
        out["x-y-vorticity"][mask[0, :, :]] = 0
        out["x-z-vorticity"][mask[:, 0, :]] = 0
        out["y-z-vorticity"][mask[:, :, 0]] = 0
    return out


def cylinder_frames(w, table, mask):
    lo, span = fixed_range(-10, 10)
    return _vortex_frames(w, (-1,), lo, span, table, mask)


def airfoil_frames(w, table, value_range):
    lo, span = fixed_range(*value_range)
    return _vortex_frames(w, (-2, -1), lo, span, table, None)


def tcf_frames(u, w, wall_row, velocity_max, table_velocity, table_vorticity):
    """tcf_env.py:679-751 on the simulation grid: ``wall_row`` is the UNFLIPPED cell row of the wall-parallel pictures.  ``u``, ``w``
    ``[3, z, y, x]`` of one env."""
    speed = np.flip(norm(u), axis=(-2, -1))
    vort = np.flip(np.asarray(w, np.float32), axis=(-2, -1))
    row = vort.shape[2] - 1 - wall_row
    lo, span = fixed_range(0.0, velocity_max)
    fv = lambda d: format_render_data(d, lo, span, table_velocity)
    wlo, wspan = auto_range(vort, symmetric=True)
    fw = lambda d: format_render_data(d, wlo, wspan, table_vorticity)
    return {
        "x-y-velocity": fv(speed[speed.shape[0] // 2, :, :]),
        "x-z-velocity": fv(speed[:, row, :]),
        "y-z-velocity": fv(speed[:, :, speed.shape[2] // 2].T),
        "x-y-vorticity": fw(vort[2, vort.shape[0] // 2, :, :]),         # tcf_env.py:745-747 on [3, z, y, x]: z plane 3 // 2 = 1,
        "x-z-vorticity": fw(vort[1, :, row, :]),
        "y-z-vorticity": fw(vort[0, :, :, vort.shape[2] // 2].T),         # x index ny // 2
    }
