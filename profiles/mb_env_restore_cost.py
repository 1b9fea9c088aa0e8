"""What a per-env reset of a multi-block env costs: 64 envs of ``CylinderJet2D-easy-v0`` at its default mesh.  ``reset_mesh_envs`` of 1,
8 and 64 envs (without randomisation: the one restore launch, the zero action on the chosen envs' boundary values, the observation)
and the bare ``MultiBlockDomain.RestoreEnvs`` of the same envs with and without the reset noise, beside what a single diverged env
cost before -- a ``MultiBlockDomain.Restore`` of the whole batch.  Host clock around work that ends in a synchronise, warm-up first,
the forms alternated inside every repetition; medians and the 10 / 90 % quantiles are written to
``profiles/mb_env_restore_cost.json``.  There is no bar to meet: the number is a record.  What is fixed is structural: one upload and
one kernel launch per ``RestoreEnvs`` (``csrc/fg_mb_envrestore.hip``).

    python profiles/mb_env_restore_cost.py [--reps 200] [--out profiles/mb_env_restore_cost.json]
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
    ap.add_argument("--development-steps", type=int, default=20, help="sim steps of the developed state (the cost does not depend on it)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "mb_env_restore_cost.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    env = fluidgym_amd.make("CylinderJet2D-easy-v0", num_envs=args.envs, load_domain_statistics=False, randomize_initial_state=False,
                            initial_domain_steps=args.development_steps)
    env.reset(seed=0)
    gen = torch.Generator().manual_seed(0)
    act = lambda: (torch.rand(env._zero_action.shape, generator=gen) * 2 - 1).to(env.cuda_device)
    for _ in range(3):
        env._n_steps = 0
        env.step(act())
    dom = env._domain
    snap = dom.Clone()
    counts = sorted({1, min(8, args.envs), args.envs})
    chosen = {n: list(range(0, args.envs, args.envs // n))[:n] for n in counts}
    env.reset_mesh_envs([0], randomize=False)        # builds the bank (env 0 of the developed state)
    bank = env.mesh_state_bank
    sigma = env._mesh_reset_sigma
    jobs = {"full_restore": lambda: dom.Restore(snap)}
    for n in counts:
        jobs[f"reset_mesh_envs_{n}"] = lambda e=chosen[n]: env.reset_mesh_envs(e, randomize=False)
        jobs[f"restore_envs_{n}"] = lambda e=chosen[n]: dom.RestoreEnvs(bank, e)
        jobs[f"restore_envs_noise_{n}"] = lambda e=chosen[n]: dom.RestoreEnvs(bank, e, noise=(0, sigma, sigma, [0] * len(e)))
    for _ in range(10):                              # warm-up: code objects, allocator
        for j in jobs.values():
            j()
    ms = {k: [] for k in jobs}
    for _ in range(args.reps):
        for k, j in jobs.items():                    # the forms alternate inside every repetition
            ms[k].append(timed(j))
    out = {"shape": {"envs": args.envs, "velocity": list(dom.velocity.shape), "pressure": list(dom.pressure.shape),
                     "boundary_velocity": list(dom.boundary_velocity.shape), "bank_states": bank.size},
           "device": torch.cuda.get_device_name(0),
           "clock": "host perf_counter around the call + synchronize",
           "per_restore": "one upload of the records, one kernel launch (by construction: fg_mb_restore_envs)",
           "forms": {"full_restore": "MultiBlockDomain.Restore of all envs (what one diverged env cost before)",
                     "reset_mesh_envs_N": "reset_mesh_envs of N envs, randomize=False",
                     "restore_envs_N": "MultiBlockDomain.RestoreEnvs of N envs, no noise",
                     "restore_envs_noise_N": "MultiBlockDomain.RestoreEnvs of N envs with the reset noise"}}
    for k, v in ms.items():
        out[k] = summarise(v)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
