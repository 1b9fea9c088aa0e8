"""NumPy fp64 restatements of the two baseline controllers (``fluidgym_amd/csrc/fg_baselines.hip``).  They take the
field the kernel takes (fp32 or fp64), convert it to fp64 and evaluate the formulas of the header with NumPy's own sums."""
import numpy as np


def opposition_action(v, rows, gain, actor):
    """``v [B, nz, ny, nx]`` (the wall-normal velocity) -> ``action [B, n_walls, nx / actor, nz / actor]`` in fp64:
    ``gain[w] (P[i, j] - m)`` with ``m`` the mean over the plane ``y = rows[w]`` and ``P[i, j]`` the mean over the patch
    ``x in [i actor, (i + 1) actor)``, ``z in [j actor, (j + 1) actor)`` (one z row per patch where ``nz = 1``)."""
    v = np.asarray(v, np.float64)
    B, nz, ny, nx = v.shape
    az = actor if nz > 1 else 1
    out = np.empty((B, len(rows), nx // actor, nz // az))
    for w, (r, g) in enumerate(zip(rows, gain)):
        plane = v[:, :, r, :]                                                                  # [B, nz, nx]
        P = plane.reshape(B, nz // az, az, nx // actor, actor).mean(axis=(2, 4))               # [B, j, i]
        out[:, w] = g * (P - plane.mean(axis=(1, 2), keepdims=True)).transpose(0, 2, 1)
    return out


def pd_energy(v, wy, seg):
    """``E [B, nz / seg, nx / seg]``: ``sum_y wy[y]`` times the mean of ``v [B, nz, ny, nx]`` over the heater's cells in (z, x)."""
    v = np.asarray(v, np.float64)
    B, nz, ny, nx = v.shape
    sz = seg if nz > 1 else 1
    col = v.reshape(B, nz // sz, sz, ny, nx // seg, seg).mean(axis=(2, 5))                     # [B, hz, ny, hx]
    return np.einsum("bzyx,y->bzx", col, np.asarray(wy, np.float64))


class PDController:
    """The state machine of ``fg_baseline_pd``: ``action = -(kp E + kd_over_dt (E - E_previous))``, the second term zero for an env
    whose ``first`` flag is set; a call stores ``E`` and clears the flags."""

    def __init__(self, batch, kp, kd_over_dt):
        self.kp, self.kd_over_dt = float(kp), float(kd_over_dt)
        self.first = np.ones(batch, bool)
        self.e = None

    def reset(self, envs=None):
        self.first[slice(None) if envs is None else list(envs)] = True

    def action(self, v, wy, seg):
        E = pd_energy(v, wy, seg)
        prev = E if self.e is None else self.e
        d = np.where(self.first[:, None, None], 0.0, self.kd_over_dt * (E - prev))
        self.e, self.first[:] = E, False
        return -(self.kp * E + d)
