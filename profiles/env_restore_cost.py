"""What a per-env reset costs at the headline shape (64 envs of the 256 x 128 channel): ``reset_envs`` of 1, 8 and 64 envs (without
randomisation: the restore launches, the per-env solver-state reset, the zero action on the chosen envs' boundary values and the
observation) and the bare ``Domain.RestoreEnvs`` of the same envs, beside what a single diverged env cost before -- a full
``Domain.Restore`` of all 64 envs plus ``reset_solver_state``.  Host clock around work that ends in a synchronise, warm-up first, the
forms alternated inside every repetition; medians and the 10 / 90 % quantiles are written to ``profiles/env_restore_cost.json``.
There is no bar to meet: the number is a record.

    python profiles/env_restore_cost.py [--reps 200] [--out profiles/env_restore_cost.json]
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
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "env_restore_cost.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    env = fluidgym_amd.make("ChannelJet2D-v0", num_envs=args.envs, load_domain_statistics=False, randomize_initial_state=False)
    env.reset(seed=0)
    gen = torch.Generator().manual_seed(0)
    act = lambda: (torch.rand(env._zero_action.shape, generator=gen) * 2 - 1).to(env.cuda_device)
    for _ in range(5):
        env._n_steps = 0
        env.step(act())
    dom = env._domain
    snap = dom.Clone()
    counts = sorted({1, min(8, args.envs), args.envs})
    chosen = {n: list(range(0, args.envs, args.envs // n))[:n] for n in counts}
    env.reset_envs([0], randomize=False)        # builds the bank (one generated state)
    bank = env.state_bank
    jobs = {"full_restore": lambda: (dom.Restore(snap), dom.solver.reset_solver_state())}
    for n in counts:
        jobs[f"reset_envs_{n}"] = lambda e=chosen[n]: env.reset_envs(e, randomize=False)
        jobs[f"restore_envs_{n}"] = lambda e=chosen[n]: dom.RestoreEnvs(bank, e, [0] * len(e))
    for _ in range(10):                         # warm-up: code objects, allocator
        for j in jobs.values():
            j()
    ms = {k: [] for k in jobs}
    for _ in range(args.reps):
        for k, j in jobs.items():               # the forms alternate inside every repetition
            ms[k].append(timed(j))
    u, p = env._statistics_fields()
    out = {"shape": {"envs": args.envs, "velocity": list(u.shape), "pressure": list(p.shape), "bank_states": bank.size,
                     "fields_per_restore": 2 + len(bank.bvel) + len(bank.bscal) + sum(k in bank.fields for k in ("scalar", "velocity_source"))},
           "device": torch.cuda.get_device_name(0),
           "clock": "host perf_counter around the call + synchronize",
           "forms": {"full_restore": "Domain.Restore of all envs + reset_solver_state (what one diverged env cost before)",
                     "reset_envs_N": "FluidEnv.reset_envs of N envs, randomize=False", "restore_envs_N": "Domain.RestoreEnvs of N envs"}}
    for k, v in ms.items():
        out[k] = summarise(v)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
