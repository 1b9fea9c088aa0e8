"""Golden values for the plane spectra from the reference's importable Python.

``simulation/pict/data/online_statistics.py`` is imported by file path through the loader of ``make_golden_plane_stats.py``.  Three
fp64 samples of velocity ``[2, 3, 8, 6, 16]`` (two envs, nz = 8, ny = 6, nx = 16) go through

    PSDOnline_Torch(total_dims=5, fft_dims=[2, 4], fft_sizes=[8, 16], mean_dims=[0], planes=[0, 2], planes_dim=3,
                    planes_symmetric=True)

as ``VelocityStats.record_vel_stats`` feeds it (``TCF_tools.py:445-459, 1491-1500``): ``n = 12``, ``fft [3, 4, 2, 8]``.  Written: the
inputs, ``n``, ``fft``, the outputs of ``get_phi`` for one ``(phys_sizes, nu, utau)``, the key names of the npz its ``save`` writes
and the parameters of its JSON file.  Data only.

    python tests/golden/make_golden_plane_spectra.py <reference>/src/fluidgym  ->  tests/golden/reference_plane_spectra.npz
"""
import json
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden_plane_stats import load_reference_statistics  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
PHYS_SIZES, NU, UTAU = [1.5, 3.0], 2.5e-3, 0.06


def main():
    S = load_reference_statistics(sys.argv[1])
    rng = np.random.default_rng(2026)
    shape = (3, 2, 3, 8, 6, 16)                                   # samples, then [B, 3, Z, Y, X]
    shear = np.linspace(0.2, 1.0, 6).reshape(1, 1, 1, 1, 6, 1) * np.array([1.0, 0.05, -0.1]).reshape(1, 1, 3, 1, 1, 1)
    z, x = np.arange(8).reshape(1, 1, 1, 8, 1, 1), np.arange(16).reshape(1, 1, 1, 1, 1, 16)
    wave = 0.3 * np.cos(2 * np.pi * (2 * x / 16 + z / 8)) + 0.2 * np.sin(2 * np.pi * 3 * x / 16)
    velocity = shear + wave + 0.25 * rng.standard_normal(shape)
    psd = S.PSDOnline_Torch(total_dims=5, fft_dims=[2, 4], fft_sizes=[8, 16], mean_dims=[0], planes=[0, 2], planes_dim=3,
                            planes_symmetric=True)
    for s in range(3):
        psd.update_from_data(torch.from_numpy(velocity[s]))
    lambdas, phi = psd.get_phi(PHYS_SIZES, NU, UTAU)
    with tempfile.TemporaryDirectory() as d:
        psd.save(d, "PSD")
        with np.load(os.path.join(d, "PSD.npz")) as f:
            keys = np.array(sorted(f.keys()))
        with open(os.path.join(d, "PSD.json")) as f:
            params = json.load(f)
    out = {"velocity": velocity, "n": np.asarray(psd.n), "fft": psd.fft.numpy(), "phi": phi.numpy(), "lambda_z": np.asarray(lambdas[0]),
           "lambda_x": np.asarray(lambdas[1]), "phys_sizes": np.asarray(PHYS_SIZES), "nu": np.asarray(NU), "utau": np.asarray(UTAU),
           "keys_psd": keys, "json_names": np.array(sorted(params)), "json_values": np.array(json.dumps(params, sort_keys=True))}
    for k, v in out.items():
        print(k, v.shape, v.dtype)
    np.savez_compressed(os.path.join(OUT, "reference_plane_spectra.npz"), **out)


if __name__ == "__main__":
    main()
