"""NumPy restatement of ``fg_mb_restore_envs`` (``fluidgym_amd/csrc/fg_mb_envrestore.hip``), built from what a
block tells about itself -- ``cell_offset``, ``size``, ``boundary_slot0`` -- and the noise stream of ``tests/obs_noise_ref.py``.  The
kernel is held to these bits."""
import numpy as np

from tests import obs_noise_ref as R

STEP_WORD = 0xFFFFFFFF      # the fourth counter word of the reset noise: a step count the observation noise never reaches


def source_plane(nz, flip_z, shift_z):
    """``zs`` of every destination plane ``z``: ``(z - shift) mod nz``, mirrored when ``flip_z``."""
    zs = (np.arange(nz) - int(shift_z)) % nz
    return nz - 1 - zs if flip_z else zs


def segments(blocks, dims, nz):
    """``(first, plane, planes, is_face)`` of every block's cells and every FIXED face's slots; ``nz``: the span symmetry (None: every
    segment is one plane)."""
    cells, faces = [], []
    for blk in blocks:
        n = int(np.prod(blk.size))
        planes = nz if nz else 1
        cells.append((blk.cell_offset, n // planes, planes, False))
        for f in range(2 * dims):
            if blk.boundary_slot0[f] >= 0:
                m = n // blk.size[f >> 1]
                faces.append((blk.boundary_slot0[f], m // planes, planes, True))
    return cells + faces


def source_index(blocks, dims, nz, n_cells, n_slots, flip_z, shift_z):
    """For every destination cell and slot the source cell and slot of one record: two index arrays."""
    cell, slot = np.arange(n_cells), np.arange(max(n_slots, 1))
    for first, plane, planes, is_face in segments(blocks, dims, nz):
        zs = source_plane(planes, flip_z, shift_z)
        idx = first + zs[:, None] * plane + np.arange(plane)[None, :]
        (slot if is_face else cell)[first:first + plane * planes] = idx.reshape(-1)
    return cell, slot


def restore_ref(blocks, dims, nz, velocity, pressure, boundary, bank_v, bank_p, bank_b, records, noise=None):
    """The call on host arrays: ``velocity [B, d, N]``, ``pressure [B, N]``, ``boundary [B, d, NB]`` and the banks ``[S, ...]``;
    ``records``: ``(env, src, flip_z, shift_z)``; ``noise``: None or ``(seed, sigma_velocity, sigma_pressure, episodes)``.  Returns the
    three arrays after the call; the inputs are not changed."""
    v, p, b = velocity.copy(), pressure.copy(), boundary.copy()
    N, NB = v.shape[-1], b.shape[-1]
    dtype = 0 if v.dtype == np.float32 else 1
    for k, (env, src, flip_z, shift_z) in enumerate(records):
        cell, slot = source_index(blocks, dims, nz, N, NB, flip_z, shift_z)
        for c in range(dims):
            negate = bool(flip_z) and c == 2
            val = -bank_v[src, c, cell] if negate else bank_v[src, c, cell]
            if noise is not None:
                z = R.normals(N, c, env, noise[3][k], STEP_WORD, noise[0])
                val = R.add_noise(val, noise[1], z, dtype)
            v[env, c] = val
            b[env, c] = -bank_b[src, c, slot] if negate else bank_b[src, c, slot]
        val = bank_p[src, cell]
        if noise is not None:
            val = R.add_noise(val, noise[2], R.normals(N, dims, env, noise[3][k], STEP_WORD, noise[0]), dtype)
        p[env] = val
    return v, p, b
