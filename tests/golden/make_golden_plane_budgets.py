"""Golden values for the Reynolds-stress budgets from the reference's importable Python.

``simulation/pict/data/online_statistics.py`` is imported by file path with the stub modules of ``make_golden_plane_stats.py``.
Three fp64 samples of velocity ``[1, 3, 4, 5, 6]``, pressure ``[1, 1, 4, 5, 6]`` and source ``[1, 3, 4, 5, 6]`` with a sheared mean
that drifts between the samples, on a grid with a tanh-refined y and uniform x and z (``grid_coordinates [1, 3, Z, Y, X]``,
``u_wall=None``), go through ``TurbulentEnergyBudgetsOnlineParallel_Torch`` with ``with_forcing=False`` (prefix ``nf_``) and
``with_forcing=True`` (prefix ``f_``).  Written: the inputs and coordinates, every mean and every raw moment of ``moments_data`` and of
the three ``moments_data_grad``, the outputs of ``production``, ``dissipation``, ``turbulent_transport``,
``velocity_pressure_gradient`` and ``velocity_forcing`` for ``(i, j)`` in ``(0, 0), (1, 1), (2, 2), (0, 1)``, and the key names each
``save`` writes.  The reference's merge of third-order sums is not right: the third-order moments and
``turbulent_transport`` are recorded, the tests hold them against a one-shot evaluation instead.  Data only.

    python tests/golden/make_golden_plane_budgets.py <reference>/src/fluidgym  ->  tests/golden/reference_plane_budgets.npz
"""
import os
import sys
import tempfile

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
from make_golden_plane_stats import load_reference_statistics  # noqa: E402

PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1))


def main():
    S = load_reference_statistics(sys.argv[1])
    rng = np.random.default_rng(2026)
    nz, ny, nx = 4, 5, 6
    x = (np.arange(nx) + 0.5) * 0.5
    z = (np.arange(nz) + 0.5) * 0.25
    e = np.tanh(1.5 * np.linspace(-1, 1, ny + 1)) / np.tanh(1.5)              # tanh-refined edges between the walls at -1 and 1
    y = 0.5 * (e[1:] + e[:-1])
    grid = np.stack(np.broadcast_arrays(x.reshape(1, 1, nx), y.reshape(1, ny, 1), z.reshape(nz, 1, 1)))[None]   # [1, 3, Z, Y, X]
    shape = (3, 1, 3, nz, ny, nx)                                             # samples, then [1, 3, Z, Y, X]
    shear = (1.0 - y ** 2).reshape(1, 1, 1, 1, ny, 1) * np.array([1.0, 0.05, -0.1]).reshape(1, 1, 3, 1, 1, 1)
    drift = np.array([0.0, 0.3, -0.2]).reshape(3, 1, 1, 1, 1, 1)              # the plane means move between the samples
    velocity = shear + drift + 0.25 * rng.standard_normal(shape)
    pressure = 0.5 + drift[:, :, :1] + 0.1 * rng.standard_normal((3, 1, 1, nz, ny, nx)) ** 3
    source = 0.1 * shear - 0.5 * drift + 0.05 * rng.standard_normal(shape)
    out = {"velocity": velocity, "pressure": pressure, "source": source, "x": x, "y": y, "z": z}
    for forcing, pre in ((False, "nf_"), (True, "f_")):
        acc = S.TurbulentEnergyBudgetsOnlineParallel_Torch(avg_dims=[0, 2], grid_coordinates=torch.from_numpy(grid),
                                                           with_forcing=forcing, u_wall=None)
        for s in range(3):
            acc.update_from_data(torch.from_numpy(velocity[s]), torch.from_numpy(pressure[s]), torch.from_numpy(source[s]) if forcing else None)
        m = acc.moments_data
        out[pre + "n"] = np.asarray(m.data.n)
        for c in range(m.max_channels):
            out[pre + "mean_%d" % c] = m.get_mean(c, squeeze=False).numpy()
        for k in sorted(m.moments):
            out[pre + "moment_" + "_".join(str(v) for v in k)] = m.get_moment(k, squeeze=False).numpy()
        for g, mg in enumerate(acc.moments_data_grad):
            assert mg.data.n == m.data.n
            for c in range(3):
                out[pre + "grad%d_mean_%d" % (g, c)] = mg.get_mean(c, squeeze=False).numpy()
            for k in sorted(mg.moments):
                out[pre + "grad%d_moment_" % g + "_".join(str(v) for v in k)] = mg.get_moment(k, squeeze=False).numpy()
        for i, j in PAIRS:
            terms = ["production", "dissipation", "turbulent_transport", "velocity_pressure_gradient"] + (["velocity_forcing"] if forcing else [])
            for t in terms:
                out[pre + "%s_%d%d" % (t, i, j)] = getattr(acc, t)(i, j).numpy()
        with tempfile.TemporaryDirectory() as d:
            acc.save(d, save_steps=False)
            assert sorted(os.listdir(d)) == ["budgets_grad_0000.npz", "budgets_grad_0001.npz", "budgets_grad_0002.npz", "budgets_moments.npz"]
            for name in ("budgets_moments.npz", "budgets_grad_0001.npz"):
                with np.load(os.path.join(d, name)) as zf:
                    out[pre + "keys_" + name[8:-4]] = np.array(sorted(zf.keys()))
    for k, v in out.items():
        print(k, v.shape, v.dtype)
    np.savez_compressed(os.path.join(OUT, "reference_plane_budgets.npz"), **out)


if __name__ == "__main__":
    main()
