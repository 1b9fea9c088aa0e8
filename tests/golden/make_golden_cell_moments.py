"""Golden values for the per-cell flow statistics of the multi-block envs from the reference's importable Python.

``simulation/pict/data/online_statistics.py`` is imported by file path with the stub of ``make_golden_plane_stats.py``.  Three fp64
samples of a 2-D block (velocity ``[1, 2, 3, 5]``, pressure ``[1, 1, 3, 5]``) and of a 3-D block (``[1, 3, 4, 3, 5]``,
``[1, 1, 4, 3, 5]``), a smooth mean plus seeded noise, go per sample, as a run script would feed them, through

    WelfordOnlineParallel_Torch([0]) / ([0, 2])              velocity, pressure              n, mean, sum_squares
    CovarianceOnlineParallel_Torch([0]) / ([0, 2])           every pair of velocity components   n, mean_x, mean_y, C

Written: the inputs, the results, and the sorted key names each class's ``save`` puts into its file.  Data only.

    python tests/golden/make_golden_cell_moments.py <reference>/src/fluidgym  ->  tests/golden/reference_cell_moments.npz
"""
import os
import sys

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
from make_golden_plane_stats import load_reference_statistics, saved_keys  # noqa: E402


def main():
    S = load_reference_statistics(sys.argv[1])
    rng = np.random.default_rng(2026)
    out = {}
    for tag, d, spatial, dims in (("d2", 2, (3, 5), [0]), ("d3", 3, (4, 3, 5), [0, 2])):
        ny, nx = spatial[-2:]
        smooth = (np.linspace(0.2, 1.1, ny)[:, None] * np.cos(np.linspace(0.0, 1.5, nx))[None, :])           # [ny, nx]
        scale = np.array([1.0, -0.2, 0.1][:d]).reshape((1, 1, d) + (1,) * len(spatial))
        drift = np.array([0.0, 0.3, -0.2]).reshape((3, 1, 1) + (1,) * len(spatial))                        # the means move between samples
        velocity = smooth * scale + drift + 0.25 * rng.standard_normal((3, 1, d) + spatial)
        pressure = 0.5 - smooth + drift + 0.1 * rng.standard_normal((3, 1, 1) + spatial) ** 3
        vel, prs = S.WelfordOnlineParallel_Torch(dims), S.WelfordOnlineParallel_Torch(dims)
        pairs = [(a, b) for a in range(d) for b in range(a + 1, d)]
        cov = {ab: S.CovarianceOnlineParallel_Torch(dims) for ab in pairs}
        for s in range(3):
            u, p = torch.from_numpy(velocity[s]), torch.from_numpy(pressure[s])
            vel.update_from_data(u)
            prs.update_from_data(p)
            for (a, b), c in cov.items():
                c.update_from_data(u[:, a:a + 1], u[:, b:b + 1])
        out.update({f"{tag}_velocity": velocity, f"{tag}_pressure": pressure,
                    f"{tag}_vel_n": np.asarray(vel.n), f"{tag}_vel_mean": vel.mean.numpy(), f"{tag}_vel_sum_squares": vel.sum_squares.numpy(),
                    f"{tag}_p_n": np.asarray(prs.n), f"{tag}_p_mean": prs.mean.numpy(), f"{tag}_p_sum_squares": prs.sum_squares.numpy()})
        for (a, b), c in cov.items():
            ab = "uvw"[a] + "uvw"[b]
            out.update({f"{tag}_cov_{ab}_n": np.asarray(c.n), f"{tag}_cov_{ab}_mean_x": c.mean_x.numpy(),
                        f"{tag}_cov_{ab}_mean_y": c.mean_y.numpy(), f"{tag}_cov_{ab}_C": c.C.numpy()})
        out[f"{tag}_keys_welford"] = saved_keys(vel.save)
        out[f"{tag}_keys_covariance"] = saved_keys(cov[(0, 1)].save)
    for k, v in out.items():
        print(k, v.shape, v.dtype)
    np.savez_compressed(os.path.join(OUT, "reference_cell_moments.npz"), **out)


if __name__ == "__main__":
    main()
