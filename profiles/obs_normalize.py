"""What the running normalisation (``fluidgym_amd/wrappers/normalize.py``, ``csrc/fg_obsnorm.hip``) costs per wrapped
``step()``, at two shapes: ``RBC2D-easy-v0`` x 64 envs (few rows of many elements) and the multi-agent ``TCFSmall3D-both-easy-v0`` x 8 envs
(many rows of few elements).  The shapes and dtypes are those of the env's own spaces (the env is built on the CPU device for them, which
simulates nothing); the tensors are random and replayed by a stub, so a wrapped ``step()`` here is the wrapper's work alone:

* the kernel launches of one ``step()`` (counted by ``torch.profiler``; ``null`` with the reason where the profiler is not usable), for
  ``NormalizeObservation`` with ``pool="element"`` and ``pool="key"`` and for ``NormalizeReward``;
* its host-clock time: the mean over ``--calls`` back-to-back calls with one synchronisation at the end, and the median of single calls
  each followed by a synchronisation;
* the same update and normalisation written in plain torch ops in fp64 (what a user would write otherwise), counted and timed the same way.

There is no bar to meet: the numbers are a record, written to ``profiles/obs_normalize.json``.

    python profiles/obs_normalize.py [--calls 200] [--out profiles/obs_normalize.json]
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
from fluidgym_amd.wrappers import FluidWrapper, NormalizeObservation, NormalizeReward  # noqa: E402

EPS = 1e-8


def count_launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile

        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if str(e.device_type).endswith("CUDA")]
        return {"launches": len(names), "kernels": sorted(set(names))}
    except Exception as exc:      # noqa: BLE001 -- a record, not a check: say why there is no count
        return {"launches": None, "reason": f"{type(exc).__name__}: {exc}"}


def host_time(fn, calls):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    stream_us = 1e6 * (time.perf_counter() - t0) / calls
    single = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        single.append(1e6 * (time.perf_counter() - t0))
    return {"back_to_back_mean_us": stream_us, "single_call_median_us": float(np.median(single)), "calls": calls}


class Replay(FluidWrapper):
    """The env's surface with a fixed observation and reward on the GPU: nothing is simulated."""

    def __init__(self, env, obs, reward):
        super().__init__(env)
        self._obs, self._reward = obs, reward

    def reset(self, seed=None, randomize=None):
        return self._obs, {}

    def step(self, action):
        return self._obs, self._reward, False, False, {}


class TorchNormalizer:
    """The same record and the same formulas in plain torch ops (fp64), one record per key."""

    def __init__(self, pooled):
        self.pooled, self.n, self.rec = pooled, 0, {}

    def __call__(self, obs, rows):
        out = {}
        for k, t in obs.items():
            x = t.reshape(rows, -1).double()
            m = x.numel() if self.pooled else rows
            n_a = self.n * (x.shape[1] if self.pooled else 1)
            mean_b = x.mean() if self.pooled else x.mean(dim=0)
            d = x - mean_b
            m2_b = (d * d).sum() if self.pooled else (d * d).sum(dim=0)
            if k not in self.rec:
                mean, m2 = mean_b, m2_b
            else:
                mean_a, m2_a = self.rec[k]
                delta = mean_b - mean_a
                mean = mean_a + delta * (m / (n_a + m))
                m2 = m2_a + m2_b + delta * delta * (n_a * m / (n_a + m))
            self.rec[k] = (mean, m2)
            out[k] = ((x - mean) * torch.rsqrt(m2 / (n_a + m) + EPS)).to(t.dtype).reshape(t.shape)
        self.n += rows
        return out


class TorchReturn:
    def __init__(self, gamma):
        self.gamma, self.n, self.G, self.rec = gamma, 0, None, None

    def __call__(self, reward):
        r = reward.reshape(-1).double()
        self.G = r if self.G is None else self.gamma * self.G + r
        m = r.numel()
        mean_b = self.G.mean()
        d = self.G - mean_b
        m2_b = (d * d).sum()
        if self.rec is None:
            mean, m2 = mean_b, m2_b
        else:
            delta = mean_b - self.rec[0]
            mean = self.rec[0] + delta * (m / (self.n + m))
            m2 = self.rec[1] + m2_b + delta * delta * (self.n * m / (self.n + m))
        self.rec, self.n = (mean, m2), self.n + m
        return (r * torch.rsqrt(m2 / self.n + EPS)).to(reward.dtype).reshape(reward.shape)


def workload(env_id, num_envs, args, **kw):
    env = fluidgym_amd.make(env_id, num_envs=num_envs, cuda_device=torch.device("cpu"), **kw)
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    lead = (num_envs, env.n_agents) if env.use_marl else (num_envs,)
    obs = {k: torch.randn(lead + tuple(s.shape), device=dev, generator=g, dtype=torch.float32) for k, s in env.observation_space.spaces.items()}
    reward = torch.randn(lead, device=dev, generator=g, dtype=torch.float32)
    rows = int(np.prod(lead))
    res = {"num_envs": num_envs, "marl": bool(env.use_marl), "rows": rows,
           "elements_per_row": {k: int(v.numel() // rows) for k, v in obs.items()}}
    replay = Replay(env, obs, reward)
    for pool in ("element", "key"):
        w = NormalizeObservation(replay, pool=pool)
        w.reset()
        entry = count_launches(lambda: w.step(None))
        entry.update(host_time(lambda: w.step(None), args.calls))
        ref = TorchNormalizer(pool == "key")
        ref(obs, rows)
        plain = count_launches(lambda: ref(obs, rows))
        plain.update(host_time(lambda: ref(obs, rows), args.calls))
        res["observation_" + pool] = {"wrapper": entry, "plain_torch": plain}
    w = NormalizeReward(replay, gamma=0.99)
    w.step(None)
    entry = count_launches(lambda: w.step(None))
    entry.update(host_time(lambda: w.step(None), args.calls))
    ref = TorchReturn(0.99)
    ref(reward)
    plain = count_launches(lambda: ref(reward))
    plain.update(host_time(lambda: ref(reward), args.calls))
    res["reward"] = {"wrapper": entry, "plain_torch": plain}
    print(env_id, json.dumps(res))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "obs_normalize.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    out = {"device": torch.cuda.get_device_name(0), "clock": "time.perf_counter on the host",
           "tensors": "random, at the shapes of the env's spaces; a stub replays them, so a step is the wrapper's work alone"}
    out["RBC2D-easy-v0 x 64"] = workload("RBC2D-easy-v0", 64, args)
    out["TCFSmall3D-both-easy-v0 x 8 (multi-agent)"] = workload("TCFSmall3D-both-easy-v0", 8, args)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
