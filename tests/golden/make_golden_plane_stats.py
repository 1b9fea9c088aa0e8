"""Golden values for the plane-averaged flow statistics from the reference's importable Python.

``simulation/pict/data/online_statistics.py`` is imported by file path with a stub module for its one package import (``ttonp`` /
``ntonp`` of ``pict.util.output``).  Three fp64 samples of velocity ``[1, 3, 4, 3, 10]`` and pressure ``[1, 1, 4, 3, 10]`` with a
sheared mean profile go through

    WelfordOnlineParallel_Torch([2, 4])            velocity, pressure      n, mean, sum_squares
    CovarianceOnlineParallel_Torch([2, 4])         u, v                    n, mean_x, mean_y, C
    MultivariateMomentsOnlineParallel_Torch        u, v, w, p, all ten second-order moments, avg_dims [0, 2]

as ``VelocityStats.record_vel_stats`` feeds them (``TCF_tools.py:1480-1507``).  Only order 2: the reference's merge of third- and
fourth-order moments is not right, those orders are tested against a one-shot evaluation.  Written: the inputs, the
results, and the key names each class's ``save`` puts into its file.  Data only.

    python tests/golden/make_golden_plane_stats.py <reference>/src/fluidgym  ->  tests/golden/reference_plane_stats.npz
"""
import importlib.util
import itertools
import os
import sys
import tempfile
import types

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))


def load_reference_statistics(ref):
    for pkg in ("fluidgym", "fluidgym.simulation", "fluidgym.simulation.pict", "fluidgym.simulation.pict.util",
                "fluidgym.simulation.pict.util.output"):
        sys.modules.setdefault(pkg, types.ModuleType(pkg))
    out = sys.modules["fluidgym.simulation.pict.util.output"]
    out.ttonp = lambda t: t.detach().cpu().numpy()
    out.ntonp = lambda v: v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
    name = "fluidgym.simulation.pict.data.online_statistics"
    spec = importlib.util.spec_from_file_location(name, f"{ref}/simulation/pict/data/online_statistics.py")
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def saved_keys(save, *args):
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "x.npz")
        save(path, *args)
        with np.load(path) as z:
            return np.array(sorted(z.keys()))


def main():
    S = load_reference_statistics(sys.argv[1])
    rng = np.random.default_rng(2025)
    shape = (3, 1, 3, 4, 3, 10)                                   # samples, then [1, 3, Z, Y, X]
    shear = np.array([0.2, 1.0, 0.3]).reshape(1, 1, 1, 1, 3, 1) * np.array([1.0, 0.05, -0.1]).reshape(1, 1, 3, 1, 1, 1)
    drift = np.array([0.0, 0.3, -0.2]).reshape(3, 1, 1, 1, 1, 1)  # the plane means move between the samples
    velocity = shear + drift + 0.25 * rng.standard_normal(shape)
    pressure = 0.5 + drift[:, :, :1] + 0.1 * rng.standard_normal((3, 1, 1, 4, 3, 10)) ** 3
    vel = S.WelfordOnlineParallel_Torch([2, 4])
    prs = S.WelfordOnlineParallel_Torch([2, 4])
    cov = S.CovarianceOnlineParallel_Torch([2, 4])
    keys2 = [k for k in itertools.product(range(3), repeat=4) if sum(k) == 2]
    mom = S.MultivariateMomentsOnlineParallel_Torch(keys2, avg_dims=[0, 2])
    for s in range(3):
        u, p = torch.from_numpy(velocity[s]), torch.from_numpy(pressure[s])
        vel.update_from_data(u)
        cov.update_from_data(u[:, :1], u[:, 1:2])
        prs.update_from_data(p)
        mom.update_from_data(torch.unbind(u[0], dim=0) + (p[0, 0],))
    out = {"velocity": velocity, "pressure": pressure,
           "vel_n": np.asarray(vel.n), "vel_mean": vel.mean.numpy(), "vel_sum_squares": vel.sum_squares.numpy(),
           "p_n": np.asarray(prs.n), "p_mean": prs.mean.numpy(), "p_sum_squares": prs.sum_squares.numpy(),
           "cov_n": np.asarray(cov.n), "cov_mean_x": cov.mean_x.numpy(), "cov_mean_y": cov.mean_y.numpy(), "cov_C": cov.C.numpy(),
           "mom_n": np.asarray(mom.data.n)}
    for c in range(4):
        out["mom_mean_%d" % c] = mom.get_mean(c, squeeze=False).numpy()
    for k in sorted(mom.moments):
        out["mom_moment_" + "_".join(str(e) for e in k)] = mom.get_moment(k, squeeze=False).numpy()
    out["keys_welford"] = saved_keys(vel.save)
    out["keys_covariance"] = saved_keys(cov.save)
    out["keys_moments"] = saved_keys(mom.save, False)
    for k, v in out.items():
        print(k, v.shape, v.dtype)
    np.savez_compressed(os.path.join(OUT, "reference_plane_stats.npz"), **out)


if __name__ == "__main__":
    main()
