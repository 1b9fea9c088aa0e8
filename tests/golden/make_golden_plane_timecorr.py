"""Golden values for the temporal two-point correlations from the reference's importable Python.

``simulation/pict/data/online_statistics.py`` is imported by file path with the stub modules of ``make_golden_plane_stats.py``.
Five fp64 samples of velocity ``[2, 3, 4, 3, 10]`` at the times ``0.1 s`` -- a sheared mean profile, a common random field that
decays by ``0.8^s`` and fresh noise of 0.1 per sample -- go through ``TemporalTwoPointCorrelation_Online_torch([2, 4])`` as
``VelocityStats.record_vel_stats`` feeds it (``TCF_tools.py:1508-1511``).  The same inputs rounded to fp32 go through the reference
in fp64 again (prefix ``f32_``): the yardstick of the fp32 library, whose only fp32 rounding is then the stored base.  Written: the
inputs, ``base_fluctuations``, ``base_rms``, ``steps_coefficients`` ``[5, 2, 3, 3]``, ``steps_time`` and the key names ``save``
writes.  Data only.

    python tests/golden/make_golden_plane_timecorr.py <reference>/src/fluidgym  ->  tests/golden/reference_plane_timecorr.npz
"""
import os
import sys

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
from make_golden_plane_stats import load_reference_statistics, saved_keys  # noqa: E402


def run(S, velocity, times):
    corr = S.TemporalTwoPointCorrelation_Online_torch([2, 4], record_steps=True)
    for u, t in zip(velocity, times):
        corr.update_from_data(torch.from_numpy(u), float(t))
    return corr


def main():
    S = load_reference_statistics(sys.argv[1])
    rng = np.random.default_rng(2025)
    steps, shape = 5, (2, 3, 4, 3, 10)
    shear = np.array([0.2, 1.0, 0.3]).reshape(1, 1, 1, 3, 1) * np.array([1.0, 0.05, -0.1]).reshape(1, 3, 1, 1, 1)
    common = 0.3 * rng.standard_normal(shape)
    velocity = np.stack([shear + 0.8 ** s * common + 0.1 * rng.standard_normal(shape) for s in range(steps)])
    times = 0.1 * np.arange(steps)
    out = {"velocity": velocity, "times": times, "velocity_f32": velocity.astype(np.float32)}
    for prefix, v in (("", velocity), ("f32_", out["velocity_f32"].astype(np.float64))):
        corr = run(S, v, times)
        out[prefix + "base_fluctuations"] = corr.base_fluctuations.numpy()
        out[prefix + "base_rms"] = corr.base_rms.numpy()
        out[prefix + "steps_coefficients"] = np.asarray(corr.steps_coefficients)
        out[prefix + "steps_time"] = np.asarray(corr.steps_time)
    out["keys_temporal"] = saved_keys(corr.save)
    for k, v in out.items():
        print(k, v.shape, v.dtype)
    print("coefficients", out["steps_coefficients"].min(), out["steps_coefficients"].max(), "base_rms >=", out["base_rms"].min())
    np.savez_compressed(os.path.join(OUT, "reference_plane_timecorr.npz"), **out)


if __name__ == "__main__":
    main()
