"""What a velocity-gradient diagnostic costs per launch (``fg_flow_diagnostic`` / ``fg_mb_flow_diagnostic``): FG_DIAG_GRADIENT and
FG_DIAG_VORTICITY on 64 envs of the 256 x 128 channel, 8 envs of a 128 x 64 x 64 box (periodic x and z, walls in y) and 64 envs of
the ``CylinderJet2D-easy-v0`` mesh, each beside a device-to-device copy that moves the same algorithmic bytes (velocity read + result
written; the copy reads half of them and writes half) on the same card.  Device events around runs of ``--launches`` back-to-back
launches, warm-up first, the forms alternated inside every repetition; medians and the 10 / 90 % quantiles per launch are written to
``profiles/flow_diag_cost.json``.  Working sets of this size stay in the last-level cache between launches, for the kernels and for
the copy alike.  There is no bar to meet: the number is a record.

    python profiles/flow_diag_cost.py [--reps 100] [--launches 10] [--out profiles/flow_diag_cost.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fluidgym_amd  # noqa: E402
from fluidgym_amd import _lib as L  # noqa: E402
from fluidgym_amd.native import NativeSolver  # noqa: E402

KINDS = {"gradient": L.FG_DIAG_GRADIENT, "vorticity": L.FG_DIAG_VORTICITY}


def summarise(us):
    us = np.asarray(us)
    return {"median_us": float(np.median(us)), "p10_us": float(np.quantile(us, 0.1)), "p90_us": float(np.quantile(us, 0.9)), "n": int(us.size)}


def workload(name, solver, velocity, dims, launches, reps):
    """Jobs of one workload: per kind the diagnostic into a preallocated result and the copy of the same algorithmic bytes."""
    torch.manual_seed(0)
    velocity.copy_(torch.randn(velocity.shape, dtype=velocity.dtype, device=velocity.device))
    jobs, meta = {}, {}
    for kname, kind in KINDS.items():
        out = solver.flow_diagnostic(kind)
        nbytes = (velocity.numel() + out.numel()) * velocity.element_size()
        src = torch.empty(nbytes // 2, dtype=torch.uint8, device=velocity.device)
        dst = torch.empty_like(src)
        jobs[kname] = lambda k=kind, o=out: solver.flow_diagnostic(k, out=o)
        jobs[kname + "_copy"] = lambda s=src, d=dst: d.copy_(s)
        meta[kname] = {"algorithmic_bytes": int(nbytes), "result_shape": list(out.shape)}
    for _ in range(5):
        for j in jobs.values():
            j()
    us = {k: [] for k in jobs}
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(reps):
        for k, j in jobs.items():               # the forms alternate inside every repetition
            start.record()
            for _ in range(launches):
                j()
            stop.record()
            stop.synchronize()
            us[k].append(1e3 * start.elapsed_time(stop) / launches)
    res = {"velocity_shape": list(velocity.shape), "dims": dims}
    for kname in KINDS:
        k, c = summarise(us[kname]), summarise(us[kname + "_copy"])
        res[kname] = dict(meta[kname], kernel=k, copy=c, ratio_to_copy=k["median_us"] / c["median_us"],
                          algorithmic_GBps=meta[kname]["algorithmic_bytes"] / k["median_us"] * 1e-3)
    print(name, json.dumps(res))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "flow_diag_cost.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    out = {"device": torch.cuda.get_device_name(0), "dtype": "float32",
           "clock": f"device events around {args.launches} back-to-back launches, per launch",
           "yardstick": "torch device-to-device copy of algorithmic_bytes / 2 (read + written = algorithmic_bytes)"}

    env = fluidgym_amd.make("ChannelJet2D-v0", num_envs=64, load_domain_statistics=False, randomize_initial_state=False)
    env.reset(seed=0)
    s = env._domain.solver
    out["channel_256x128_B64"] = workload("channel_256x128_B64", s, s.velocity, 2, args.launches, args.reps)
    env.close()

    s = NativeSolver([np.full(128, 1.0 / 32, np.float32), np.full(64, 1.0 / 32, np.float32), np.full(64, 1.0 / 32, np.float32)], 8,
                     fixed_faces=(2, 3))
    out["box_128x64x64_B8"] = workload("box_128x64x64_B8", s, s.velocity, 3, args.launches, args.reps)
    s.close()

    env = fluidgym_amd.make("CylinderJet2D-easy-v0", num_envs=64, initial_domain_steps=1, load_initial_domain=False,
                            load_domain_statistics=False, randomize_initial_state=False)
    env.reset(seed=0)
    dom = env._domain
    out["cylinder_easy_B64"] = dict(workload("cylinder_easy_B64", dom, dom.velocity, 2, args.launches, args.reps), cells=int(dom.n_cells))
    env.close()

    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
