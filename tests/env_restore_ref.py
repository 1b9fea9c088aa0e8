"""NumPy restatement of the per-env restore (``csrc/fg_envrestore.hip``), by index arithmetic alone:

    dst[env, c, z, y, x] = sign(c) * bank[src, c, zs, y, xs]
    xs = flip_x ? nx-1 - ((x - shift_x) mod nx) : (x - shift_x) mod nx,   zs likewise with nz,
    sign(c) = -1 for component 0 under flip_x and component 2 under flip_z of a vector field, else +1.

A copy and a negation do not round: the tests compare bit for bit.  Used by the tests only."""
import numpy as np


def source_index(n: int, flip: int, shift: int) -> np.ndarray:
    """``[n]``: the source cell of every destination cell along one axis."""
    i = (np.arange(n) - int(shift)) % n
    return (n - 1 - i) if flip else i


def transform_state(state: np.ndarray, dims: int, flip_x=0, flip_z=0, shift_x=0, shift_z=0, signed=False) -> np.ndarray:
    """One state ``[C, (nz,) ny, nx]`` mirrored, then rolled.  An axis of extent 1 (the normal axis of a face array) has one cell
    and maps onto itself."""
    out = np.take(state, source_index(state.shape[-1], flip_x, shift_x), axis=-1)
    if dims == 3:
        out = np.take(out, source_index(state.shape[-3], flip_z, shift_z), axis=-3)
    else:
        assert not flip_z and not shift_z
    out = out.copy()
    if signed:
        if flip_x:
            out[0] = -out[0]
        if flip_z:
            out[2] = -out[2]
    return out


def restore_ref(dst: np.ndarray, bank: np.ndarray, dims: int, envs, src, flip_x=None, flip_z=None, shift_x=None, shift_z=None,
                signed=False) -> np.ndarray:
    """``dst [B, C, ...]`` with the envs ``envs`` replaced by transformed states of ``bank [S, C, ...]``; every other env is the
    input's, untouched."""
    n = len(envs)
    col = lambda v: [0] * n if v is None else [int(x) for x in np.broadcast_to(np.asarray(v), (n,))]
    out = dst.copy()
    for e, s, fx, fz, sx, sz in zip(envs, col(src), col(flip_x), col(flip_z), col(shift_x), col(shift_z)):
        out[e] = transform_state(bank[s], dims, fx, fz, sx, sz, signed)
    return out
