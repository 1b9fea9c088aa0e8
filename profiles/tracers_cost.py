"""What a tracer cloud costs on the single-block envs (default: ``RBC2D-baseline-v0`` x 32 with 4096 tracers per env and
``TCF3D-baseline-v0`` x 8 with 16384): env-steps/s of ``env.step`` with and without an active cloud -- the same env in one process,
the two alternated inside every repetition, timed with the host clock around ``--steps`` env steps that end in a device synchronise
-- and one ``TracerCloud.advect`` launch and one ``env.probe`` launch on their own, timed with device events around ``--inner``
back-to-back calls.  Medians and the 10 / 90 % quantiles go to ``profiles/tracers_cost.json``.  Without a cloud the step path takes
no tracer launch, so "without" is the env as it was before the tracers existed.

    python profiles/tracers_cost.py [--reps 5] [--steps 8] [--inner 20] [--out profiles/tracers_cost.json]
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


def event_ms(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def summarise(v):
    v = np.asarray(v)
    return {"median": float(np.median(v)), "p10": float(np.quantile(v, 0.1)), "p90": float(np.quantile(v, 0.9)), "n": int(v.size)}


def measure(env_id, envs, tracers, args):
    env = fluidgym_amd.make(env_id, num_envs=envs, load_initial_domain=False, load_domain_statistics=False)      # (the randomised, developed reset)
    env.reset(seed=0)
    zero = torch.zeros(env._zero_action.shape, device=env.cuda_device)

    def steps_per_s():
        if env._n_steps + args.steps > env.episode_length:
            env.reset(seed=0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            env.step(zero)
        torch.cuda.synchronize()
        return envs * args.steps / (time.perf_counter() - t0)

    env.step(zero)                                   # warm-up of both forms
    env.start_tracers(tracers, seed=0)
    env.step(zero)
    env.stop_tracers()
    rate = {"without": [], "with": []}
    for _ in range(args.reps):
        rate["without"].append(steps_per_s())
        env.start_tracers(tracers, seed=0)
        rate["with"].append(steps_per_s())
        cloud = env.stop_tracers()
    dt = env._sim_step_time()
    pts = cloud.seed_positions[0, :4096].contiguous()
    advect_ms = [event_ms(lambda: cloud.advect(dt), args.inner) for _ in range(args.reps)]
    probe_ms = [event_ms(lambda: env.probe(pts), args.inner) for _ in range(args.reps)]
    out = {"envs": envs, "tracers_per_env": tracers, "substeps": cloud.substeps, "sim_steps_per_env_step": int(env.n_sim_steps),
           "grid": [int(v) for v in env._domain.getBlock(0).velocity.shape[2:]], "lost": int(cloud.lost.sum()),
           "env_steps_per_s_without": summarise(rate["without"]), "env_steps_per_s_with": summarise(rate["with"]),
           "advect_ms": summarise(advect_ms), "probe_4096_points_ms": summarise(probe_ms)}
    out["with_over_without"] = out["env_steps_per_s_with"]["median"] / out["env_steps_per_s_without"]["median"]
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=8, help="env steps inside one timed window")
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--cases", default="RBC2D-baseline-v0:32:4096,TCF3D-baseline-v0:8:16384")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "tracers_cost.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    out = {"device": torch.cuda.get_device_name(0),
           "clock": f"host clock around {args.steps} env steps ending in a synchronise, with / without alternated; device events around "
                    f"{args.inner} back-to-back launches"}
    for case in args.cases.split(","):
        env_id, envs, tracers = case.split(":")
        out[env_id] = measure(env_id, int(envs), int(tracers), args)
        print(env_id, json.dumps(out[env_id]), flush=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
