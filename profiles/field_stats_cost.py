"""What one sample of the domain statistics costs at the headline shape (64 envs of the 256 x 128 channel): one
``FieldSummary.update`` of the velocity field (magnitude, 16.8 MB), one of the pressure field (component, 8.4 MB), in the
two-kernel form (moments, host read, histogram) and the fused form (one pass into a scratch histogram), beside one env step of the
same env.  Host clock around work that ends in a synchronise (every update reads its moments back), warm-up first, the forms
alternated inside every repetition; medians and the 10 / 90 % quantiles are written to ``profiles/field_stats_cost.json``.

    python profiles/field_stats_cost.py [--reps 200] [--out profiles/field_stats_cost.json]
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
from fluidgym_amd.simulation.field_stats import FieldSummary  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def summarise(ms):
    ms = np.asarray(ms)
    return {"median_ms": float(np.median(ms)), "p10_ms": float(np.quantile(ms, 0.1)), "p90_ms": float(np.quantile(ms, 0.9)),
            "n": int(ms.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "field_stats_cost.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    env = fluidgym_amd.make("ChannelJet2D-v0", num_envs=args.envs, load_domain_statistics=False)
    env.reset(seed=0)
    gen = torch.Generator().manual_seed(0)
    act = lambda: (torch.rand(env._zero_action.shape, generator=gen) * 2 - 1).to(env.cuda_device)
    for _ in range(5):
        env._n_steps = 0
        env.step(act())
    u, p = env._statistics_fields()
    forms = {"two_kernel": False, "fused": True}
    summaries = {(f, k): FieldSummary(fused=forms[f]) for f in forms for k in ("velocity", "pressure")}
    jobs = {(f, "velocity"): (lambda s=summaries[(f, "velocity")]: s.update(u)) for f in forms}
    jobs.update({(f, "pressure"): (lambda s=summaries[(f, "pressure")]: s.update(p, channel=0)) for f in forms})
    for _ in range(10):                         # warm-up: code objects, the first range, the scratch allocation
        for j in jobs.values():
            j()
    ms = {k: [] for k in jobs}
    step_ms = []
    for r in range(args.reps):
        for k, j in jobs.items():               # the forms alternate inside every repetition
            ms[k].append(timed(j))
        if r % 4 == 0:
            env._n_steps = 0
            a = act()
            step_ms.append(timed(lambda: env.step(a)))
            u, p = env._statistics_fields()
    # the two forms must agree on what they counted
    for k in ("velocity", "pressure"):
        a, b = summaries[("two_kernel", k)], summaries[("fused", k)]
        assert (a.range.lo, a.range.width) == (b.range.lo, b.range.width) and np.array_equal(a.histogram(), b.histogram())
    out = {"shape": {"envs": args.envs, "velocity": list(u.shape), "pressure": list(p.shape),
                     "velocity_bytes": u.numel() * u.element_size(), "pressure_bytes": p.numel() * p.element_size()},
           "device": torch.cuda.get_device_name(0), "nbins": 4096,
           "clock": "host perf_counter around update() + synchronize; every update reads its moments back",
           "env_step": summarise(step_ms)}
    for (f, k), v in ms.items():
        out.setdefault(f, {})[k + "_update"] = summarise(v)
    out["default_form"] = "fused" if FieldSummary().fused else "two_kernel"
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
