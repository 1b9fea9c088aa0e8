"""What the wall curves cost on the multi-block envs (default: ``CylinderJet2D-easy-v0`` x 64 and ``Airfoil2D-easy-v0`` x 64): one
``WallRing.distribution`` (one launch of ``fg_mb_wall_distribution``) and one ``WallMoments.update`` (one launch of
``fg_mb_wall_moments``), beside the same four channels as the tensor expression a user would write from the ring's index tables
(``forces_tensor_form``-style indexing: gathers, rolls and the arithmetic of ``compute_forces_2d`` without the sum), and beside one
sim step of the same env.  All of them are timed with device events -- around ``--inner`` back-to-back calls, around ``--sim-inner``
sim steps -- after a warm-up, alternated inside every repetition; medians and the 10 / 90 % quantiles go to
``profiles/wall_stats_cost.json``.

Every case runs in a fresh child process under its own time limit (``--limit`` seconds); the first case that fails, faults or runs
out of time ends the script with its status, and nothing more is started on the GPU.

    python profiles/wall_stats_cost.py [--reps 30] [--inner 20] [--out profiles/wall_stats_cost.json]
"""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def event_ms(fn, inner):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def summarise(ms):
    import numpy as np
    ms = np.asarray(ms)
    return {"median_ms": float(np.median(ms)), "p10_ms": float(np.quantile(ms, 0.1)), "p90_ms": float(np.quantile(ms, 0.9)),
            "n": int(ms.size)}


def tensor_form(ring, dom, nu):
    """The four channels [B, 4, layers, n] by tensor indexing: the arithmetic of ``compute_forces_2d`` per face, without the sum."""
    import torch
    ci, si = ring.cell_index.reshape(ring.nz, -1), ring.slot_index.reshape(ring.nz, -1)
    u = dom.velocity[:, :2][:, :, ci]                      # [B, 2, layers, n]
    ub = dom.boundary_velocity[:, :2][:, :, si]
    p = dom.pressure[:, ci]
    nx, ny = ring.wall_normals[0], ring.wall_normals[1]
    tx, ty = ny, -nx
    dn = (u - ub) / ring.wall_distances
    dt = (torch.roll(u, 1, -1) - torch.roll(u, -1, -1)) / (2 * ring.tangent_lengths)
    du_dx, du_dy = dn[:, 0] * nx + dt[:, 0] * tx, dn[:, 0] * ny + dt[:, 0] * ty
    dv_dx, dv_dy = dn[:, 1] * nx + dt[:, 1] * tx, dn[:, 1] * ny + dt[:, 1] * ty
    sxy = 0.5 * (du_dy + dv_dx)
    two_nu = 2 * nu
    fx = (two_nu * du_dx - p) * nx + two_nu * sxy * ny
    fy = two_nu * sxy * nx + (two_nu * dv_dy - p) * ny
    tau = (two_nu * du_dx * nx + two_nu * sxy * ny) * ny - (two_nu * sxy * nx + two_nu * dv_dy * ny) * nx
    return torch.stack([p, tau, fx, fy], dim=1)


def measure(env_id, envs, args):
    import torch

    sys.path.insert(0, os.path.dirname(HERE))
    import fluidgym_amd

    assert torch.cuda.is_available(), "this measurement needs the GPU"
    env = fluidgym_amd.make(env_id, num_envs=envs, randomize_initial_state=False, initial_domain_steps=args.initial_steps)
    env.reset(seed=0)
    env.step(torch.zeros(env._zero_action.shape, device=env.cuda_device))
    dom, ring = env._domain, env._ring
    nu = env._wall_force_args()[0]
    nu_t = float(nu) if not isinstance(nu, torch.Tensor) else nu.reshape(-1, 1, 1)
    out_t = torch.empty(envs, 4, ring.nz, ring.n_faces, dtype=dom.dtype, device=dom.device)
    acc = ring.moments(envs, dom.dtype)
    jobs = {"wall_distribution": lambda: ring.distribution(dom, nu, out=out_t), "wall_moments": lambda: acc.update(dom, nu),
            "tensor_form": lambda: tensor_form(ring, dom, nu_t)}
    for _ in range(5):
        for j in jobs.values():
            j()
    # the three agree on what they computed (same formulas in the env's dtype; the tensor form may contract and reorder)
    got, want = ring.distribution(dom, nu), tensor_form(ring, dom, nu_t)
    scale = want.abs().amax(dim=(0, 2, 3), keepdim=True)
    assert bool(((got - want).abs() <= 1e-4 * scale).all()), float(((got - want).abs() / scale).max())
    ms = {k: [] for k in jobs}
    sim_ms = []
    for _ in range(args.reps):
        for k, j in jobs.items():
            ms[k].append(event_ms(j, args.inner))
        sim_ms.append(event_ms(env._sim.single_step, args.sim_inner))
    out = {"device": torch.cuda.get_device_name(0), "envs": envs, "faces": ring.n_faces, "layers": ring.nz, "cells": dom.n_cells,
           "clock": f"device events around {args.inner} back-to-back calls, around {args.sim_inner} sim steps",
           "sim_step": summarise(sim_ms)}
    out.update({k: summarise(v) for k, v in ms.items()})
    for k in ("wall_distribution", "wall_moments"):
        out[k]["share_of_sim_step"] = out[k]["median_ms"] / out["sim_step"]["median_ms"]
    out["tensor_form_over_distribution"] = out["tensor_form"]["median_ms"] / out["wall_distribution"]["median_ms"]
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--sim-inner", type=int, default=3, help="sim steps between the two events of one sim-step timing")
    ap.add_argument("--initial-steps", type=int, default=50, help="uncontrolled steps that develop the initial state")
    ap.add_argument("--cases", default="CylinderJet2D-easy-v0:64,Airfoil2D-easy-v0:64")
    ap.add_argument("--limit", type=int, default=240, help="seconds one case may take")
    ap.add_argument("--out", default=os.path.join(HERE, "wall_stats_cost.json"))
    ap.add_argument("--case", default=None, help="(child) measure this one case and print its JSON")
    args = ap.parse_args()
    if args.case is not None:
        env_id, envs = args.case.split(":")
        print("RESULT " + json.dumps(measure(env_id, int(envs), args)), flush=True)
        return 0
    out = {}
    for case in args.cases.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--case", case, "--reps", str(args.reps), "--inner", str(args.inner),
               "--sim-inner", str(args.sim_inner), "--initial-steps", str(args.initial_steps)]
        try:
            child = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            print(f"{case}: no result within {args.limit} s; stopping", flush=True)
            return 124
        lines = [line for line in child.stdout.splitlines() if line.startswith("RESULT ")]
        if child.returncode != 0 or not lines:
            print(f"{case}: exit status {child.returncode}; stopping\n{child.stdout[-2000:]}\n{child.stderr[-4000:]}", flush=True)
            return child.returncode or 1
        out[case.split(":")[0]] = json.loads(lines[-1][len("RESULT "):])
        print(case, lines[-1][len("RESULT "):], flush=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
