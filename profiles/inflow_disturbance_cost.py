"""What the per-env unsteady inflow costs (default: ``CylinderJet2D-easy-v0`` x 64 at its default mesh): one sim step with the
disturbance off (``sim.single_step()``) and on (the one launch of ``fg_mb_inflow_disturbance`` before it, as the env's sim-step loop
issues it), and the launch alone.  All three are timed with device events -- around ``--sim-inner`` sim steps, around ``--inner``
back-to-back launches -- after a warm-up, alternated inside every repetition; medians and the 10 / 90 % quantiles go to
``profiles/inflow_disturbance_cost.json``.  There is no bar to meet: the number is a record.  What is fixed is structural: one launch
per sim step for the whole batch, one upload of ``[B, 2]`` words per env step, nothing read back.

    python profiles/inflow_disturbance_cost.py [--reps 30] [--inner 20] [--out profiles/inflow_disturbance_cost.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import fluidgym_amd  # noqa: E402


def event_ms(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def summarise(ms):
    ms = np.asarray(ms)
    return {"median_ms": float(np.median(ms)), "p10_ms": float(np.quantile(ms, 0.1)), "p90_ms": float(np.quantile(ms, 0.9)),
            "n": int(ms.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--sim-inner", type=int, default=3, help="sim steps between the two events of one sim-step timing")
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--initial-steps", type=int, default=50, help="uncontrolled steps that develop the initial state")
    ap.add_argument("--out", default=os.path.join(HERE, "inflow_disturbance_cost.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    env = fluidgym_amd.make("CylinderJet2D-easy-v0", num_envs=args.envs, load_domain_statistics=False, randomize_initial_state=False,
                            initial_domain_steps=args.initial_steps)
    env.reset(seed=0)
    env.start_inflow_disturbance(seed=0, n_streamwise=8, n_transverse=8, band=(0.05, 1.0), streamwise_rms=0.05, transverse_rms=0.02,
                                 kappa=0.25)
    env.step(torch.zeros(env._zero_action.shape, device=env.cuda_device))
    sim = env._sim

    def step_on():
        env._before_sim_step(1)          # (k > 0: no upload, as in four of the five sim steps of an env step)
        sim.single_step()

    jobs = {"sim_step_off": (sim.single_step, args.sim_inner), "sim_step_on": (step_on, args.sim_inner),
            "launch": (lambda: env._before_sim_step(1), args.inner)}
    for _ in range(3):
        for fn, _n in jobs.values():
            fn()
    ms = {k: [] for k in jobs}
    for _ in range(args.reps):
        for k, (fn, inner) in jobs.items():              # the forms alternate inside every repetition
            ms[k].append(event_ms(fn, inner))
    dom = env._domain
    out = {"device": torch.cuda.get_device_name(0), "env": "CylinderJet2D-easy-v0", "envs": args.envs, "cells": dom.n_cells,
           "boundary_slots": dom.n_boundary_faces, "inflow_slots": dom._outflow_slots(env._mesh.inflow)[1], "modes": [8, 8],
           "clock": f"device events around {args.sim_inner} sim steps, around {args.inner} back-to-back launches"}
    out.update({k: summarise(v) for k, v in ms.items()})
    out["launch_share_of_sim_step"] = out["launch"]["median_ms"] / out["sim_step_off"]["median_ms"]
    out["on_over_off"] = out["sim_step_on"]["median_ms"] / out["sim_step_off"]["median_ms"]
    env.close()
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
