"""What one sample of the per-cell flow statistics costs on the multi-block envs (default: ``CylinderJet2D-easy-v0`` x 64 and
``CylinderJet3D-easy-v0`` x 8): one ``CellMoments.update`` (one launch of ``fg_mb_cell_moments``), beside the same update as the torch
expression the reference's classes amount to (per block a mean, a full-field difference and a sum for the velocity, the pressure and
every velocity pair, merged like ``WelfordOnlineParallel_Torch`` / ``CovarianceOnlineParallel_Torch``, batched over the envs), and
beside one sim step of the same env, and beside the same launch on a copy of the fields behind unaligned pointers (scalar loads in every
block: what the 16-byte form is worth on that mesh; the planned form per block is reported).  All of them are timed with device
events -- around ``--inner`` back-to-back calls, around ``--sim-inner`` sim steps -- after a warm-up, alternated inside every
repetition; medians and the 10 / 90 % quantiles go to ``profiles/cell_moments_cost.json``.  The kernel's bytes are the
algorithm's: ``item * K * cells`` of fields plus ``2 * 8 * (K + K (K + 1) / 2)`` per column of accumulators, per env.

    python profiles/cell_moments_cost.py [--reps 30] [--inner 20] [--out profiles/cell_moments_cost.json]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fluidgym_amd  # noqa: E402
from fluidgym_amd.simulation.cell_moments import CellMoments  # noqa: E402

HBM_ACHIEVABLE_GB_S = 6300.0        # streaming rate an MI355X reaches in practice (8 TB/s peak)


def event_ms(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def planned_widths(acc, u, p):
    """Columns per thread in every block of the launch ``acc.update(u, p)`` makes (1: scalar loads)."""
    from fluidgym_amd import _lib as L
    lib = L.load_f64() if u.dtype == torch.float64 else L.load()
    out = (ctypes.c_int32 * len(acc.blocks))()
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    L.check(lib.fg_mb_cell_moments_widths(ptr(u), ptr(p), int(u.shape[2]), acc._table, len(acc.blocks), ptr(acc._dev[0]),
                                          ptr(acc._dev[1]), out), lib=lib)
    return list(out)


def unaligned(t):
    """A contiguous copy of ``t`` whose first element sits one element past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    buf[1:].copy_(t.reshape(-1))
    return buf[1:].view(t.shape)


def summarise(ms):
    ms = np.asarray(ms)
    return {"median_ms": float(np.median(ms)), "p10_ms": float(np.quantile(ms, 0.1)), "p90_ms": float(np.quantile(ms, 0.9)),
            "n": int(ms.size)}


class TorchCellMoments:
    """Per block: running mean / sum of squares of velocity and pressure and the covariance of every velocity pair over the span
    (dims = [0] of a one-env tensor in 2-D: the column is the cell), merged like the reference, all envs in one tensor."""

    def __init__(self, rec: CellMoments):
        self.rows = [tuple(int(v) for v in r) for r in rec.table]
        self.samples = 0
        self.state = [None] * len(self.rows)

    def update(self, velocity, pressure):
        for i, (off, layer, nz, _) in enumerate(self.rows):
            u = velocity[:, :, off:off + nz * layer].reshape(velocity.shape[0], -1, nz, layer)
            p = pressure[:, None, off:off + nz * layer].reshape(velocity.shape[0], 1, nz, layer)
            d = u.shape[1]
            mu, mp = torch.mean(u, dim=2, keepdim=True), torch.mean(p, dim=2, keepdim=True)
            du = u - mu
            ss, sp = torch.sum(torch.square(du), dim=2), torch.sum(torch.square(p - mp), dim=2)
            cov = [torch.sum(du[:, a] * du[:, b], dim=1) for a in range(d) for b in range(a + 1, d)]
            mu, mp = mu[:, :, 0], mp[:, :, 0]
            if self.state[i] is not None:
                m0, s0, q0, t0, c0 = self.state[i]
                n0, n1 = self.samples * nz, nz
                n, w = n0 + n1, n0 * n1 / (n0 + n1)
                dl = mu - m0
                ss, sp = s0 + ss + torch.square(dl) * w, t0 + sp + torch.square(mp - q0) * w
                pairs = [(a, b) for a in range(d) for b in range(a + 1, d)]
                cov = [c0[k] + cov[k] + dl[:, a] * dl[:, b] * w for k, (a, b) in enumerate(pairs)]
                mu, mp = (n0 * m0 + n1 * mu) / n, (n0 * q0 + n1 * mp) / n
            self.state[i] = (mu, ss, mp, sp, cov)
        self.samples += 1


def measure(env_id, envs, args):
    kw = dict(num_envs=envs, randomize_initial_state=False, initial_domain_steps=args.initial_steps)
    env = fluidgym_amd.make(env_id, **kw)
    env.reset(seed=0)
    env.step(torch.zeros(env._zero_action.shape, device=env.cuda_device))
    dom = env._domain
    u, p = dom.velocity, dom.pressure
    acc = CellMoments.for_domain(dom)
    ref = TorchCellMoments(acc)
    scalar, us, ps = CellMoments.for_domain(dom), unaligned(u), unaligned(p)
    jobs = {"cell_moments": lambda: acc.update(u, p), "cell_moments_scalar_loads": lambda: scalar.update(us, ps),
            "torch": lambda: ref.update(u, p)}
    for _ in range(5):
        for j in jobs.values():
            j()
    # the two agree on what they computed (fp32 torch against the fp64 kernel)
    got, want = acc.mean("u", 0), ref.state[0][0][:, 0].double().cpu().numpy().reshape(acc.mean("u", 0).shape)
    assert np.allclose(got, want, rtol=1e-3, atol=1e-5), float(np.abs(got - want).max())
    assert all(np.array_equal(a, b) for a, b in zip(acc._state(), scalar._state()))
    widths = planned_widths(acc, u, p)
    assert set(planned_widths(scalar, us, ps)) == {1}
    ms = {k: [] for k in jobs}
    sim_ms = []
    for r in range(args.reps):
        for k, j in jobs.items():
            ms[k].append(event_ms(j, args.inner))
        sim_ms.append(event_ms(env._sim.single_step, args.sim_inner))
    K, P, B = acc.K, acc.P, u.shape[0]
    nbytes = B * (u.element_size() * K * int((acc.table[:, 1] * acc.table[:, 2]).sum()) + 2 * 8 * (K + P) * acc.NC)
    out = {"envs": envs, "blocks": [list(s) for s, _ in acc.blocks], "cells": dom.n_cells, "columns": acc.NC, "columns_per_thread": widths,
           "algorithmic_bytes": nbytes, "sim_step": summarise(sim_ms)}
    out.update({k: summarise(v) for k, v in ms.items()})
    out["cell_moments"]["algorithmic_GB_per_s"] = nbytes / out["cell_moments"]["median_ms"] * 1e-6
    out["cell_moments"]["share_of_achievable_hbm"] = out["cell_moments"]["algorithmic_GB_per_s"] / HBM_ACHIEVABLE_GB_S
    out["cell_moments"]["share_of_sim_step"] = out["cell_moments"]["median_ms"] / out["sim_step"]["median_ms"]
    out["scalar_loads_over_kernel"] = out["cell_moments_scalar_loads"]["median_ms"] / out["cell_moments"]["median_ms"]
    out["torch_over_kernel"] = out["torch"]["median_ms"] / out["cell_moments"]["median_ms"]
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--sim-inner", type=int, default=3, help="sim steps between the two events of one sim-step timing")
    ap.add_argument("--initial-steps", type=int, default=50, help="uncontrolled steps that develop the initial state")
    ap.add_argument("--cases", default="CylinderJet2D-easy-v0:64,CylinderJet3D-easy-v0:8")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "cell_moments_cost.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    out = {"device": torch.cuda.get_device_name(0),
           "clock": f"device events around {args.inner} back-to-back calls, around {args.sim_inner} sim steps"}
    for case in args.cases.split(","):
        env_id, envs = case.split(":")
        out[env_id] = measure(env_id, int(envs), args)
        print(env_id, json.dumps(out[env_id]), flush=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
