"""What one sample of the plane-averaged flow statistics costs at the TCF shape (8 envs of 128 x 64 x 64 cells): one
``PlaneMoments.update`` of ``u, v, w, p`` at orders 2 and 4 (one launch of ``fg_plane_moments``, 67 MB read once from HBM), beside
the torch expression of the order-2 statistics a user had before (the arithmetic of the reference's ``update_from_data``: mean and
sum of squared deviations of the velocity and of the pressure, covariance of ``u, v`` -- a mean, a full-field difference and a sum
each), and beside one sim step and one env step of the same env.  Device events around ``--inner`` back-to-back calls, warm-up
first, the forms alternated inside every repetition; medians and the 10 / 90 % quantiles go to ``profiles/plane_stats_cost.json``.

    python profiles/plane_stats_cost.py [--reps 30] [--inner 10] [--out profiles/plane_stats_cost.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fluidgym_amd  # noqa: E402
from fluidgym_amd.simulation.plane_stats import PlaneMoments  # noqa: E402


def event_ms(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def summarise(ms):
    ms = np.asarray(ms)
    return {"median_ms": float(np.median(ms)), "p10_ms": float(np.quantile(ms, 0.1)), "p90_ms": float(np.quantile(ms, 0.9)),
            "n": int(ms.size)}


class TorchOrder2:
    """Running mean / sum of squares of velocity and pressure and the u, v covariance over dims (z, x), merged like the reference."""

    def __init__(self):
        self.n = 0
        self.vel = self.p = self.cov = None

    @staticmethod
    def _welford(state, n0, n1, mean, ss):
        if state is None:
            return mean, ss
        m0, s0 = state
        n = n0 + n1
        return (n0 * m0 + n1 * mean) / n, s0 + ss + torch.square(mean - m0) * (n0 * n1 / n)

    def update(self, u, p):
        n1 = u.shape[2] * u.shape[4]
        mu = torch.mean(u, dim=(2, 4), keepdim=True)
        du = u - mu
        ss = torch.sum(torch.square(du), dim=(2, 4))
        mp = torch.mean(p, dim=(2, 4), keepdim=True)
        sp = torch.sum(torch.square(p - mp), dim=(2, 4))
        c = torch.sum(du[:, 0] * du[:, 1], dim=(1, 3))
        mu, mp = mu[:, :, 0, :, 0], mp[:, :, 0, :, 0]
        if self.cov is not None:
            d = mu - self.vel[0]
            c = self.cov + c + d[:, 0] * d[:, 1] * (self.n * n1 / (self.n + n1))
        self.vel, self.p, self.cov = self._welford(self.vel, self.n, n1, mu, ss), self._welford(self.p, self.n, n1, mp, sp), c
        self.n += n1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--envs", type=int, default=8)
    ap.add_argument("--env-id", default="TCF3D-baseline-v0")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "plane_stats_cost.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    env = fluidgym_amd.make(args.env_id, num_envs=args.envs, use_marl=False, randomize_initial_state=False, load_domain_statistics=False)
    env.reset(seed=0)
    zero = torch.zeros(env._zero_action.shape, device=env.cuda_device)

    def env_step():
        env._n_steps = 0
        env.step(zero)

    env_step()
    u, p = env._block.velocity, env._block.pressure
    acc = {2: PlaneMoments(order=2), 4: PlaneMoments(order=4)}
    ref = TorchOrder2()
    jobs = {"plane_moments_order2": lambda: acc[2].update(u, p), "plane_moments_order4": lambda: acc[4].update(u, p),
            "torch_order2": lambda: ref.update(u, p)}
    for _ in range(5):
        for j in jobs.values():
            j()
    # the two agree on what they computed (fp32 torch against the fp64 kernel)
    got, want = acc[2].moment((2, 0, 0, 0)), ref.vel[1][:, 0].double().cpu().numpy()
    assert np.allclose(got, want, rtol=1e-3), float(np.abs(got / want - 1).max())
    ms = {k: [] for k in jobs}
    sim_ms, step_ms = [], []
    for r in range(args.reps):
        for k, j in jobs.items():
            ms[k].append(event_ms(j, args.inner))
        if r % 3 == 0:
            sim_ms.append(host_ms(env._sim.single_step))
        if r % 10 == 0:
            step_ms.append(host_ms(env_step))
    K, item = 4, u.element_size()
    out = {"shape": {"envs": args.envs, "velocity": list(u.shape), "pressure": list(p.shape), "sim_steps_per_env_step": env._n_sim_steps},
           "device": torch.cuda.get_device_name(0), "algorithmic_bytes": K * p.numel() * item,
           "clock": f"device events around {args.inner} back-to-back calls; sim / env step: host clock around work ending in a synchronise",
           "sim_step": summarise(sim_ms), "env_step": summarise(step_ms)}
    out.update({k: summarise(v) for k, v in ms.items()})
    for k in ("plane_moments_order2", "plane_moments_order4"):
        out[k]["algorithmic_GB_per_s"] = out["algorithmic_bytes"] / out[k]["median_ms"] * 1e-6
        out[k]["share_of_sim_step"] = out[k]["median_ms"] / out["sim_step"]["median_ms"]
    out["torch_over_kernel_order2"] = out["torch_order2"]["median_ms"] / out["plane_moments_order2"]["median_ms"]
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
