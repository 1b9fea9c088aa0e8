"""What one sample of the temporal two-point correlations costs on the two channel workloads of the bench, ``TCF3D-baseline-v0`` x 8
envs (``u, v, w``) and ``RBC2D-baseline-v0`` x 32 envs (``u, v``), fp32: one ``PlaneTimeCorrelation.update`` (one launch of
``fg_plane_timecorr``) with 1, 4 and 8 live base slots -- ``lags = stride-1 slots``, so that after ``lags`` samples every sample
stores one base and correlates with all of them -- beside one sim step and one env step of the same env with the recorder off (the
step path as it was before the recorder existed: the yardstick).  Per sample: its share of a sim step, and the bytes of the model
``(2 + live slots) K field bytes`` (the channel read in both passes -- the second one is meant to hit cache --, every live base read
or written once) per second, as a fraction of the STREAM triad that ``bench.py`` measures, taken here in the same process.  Device
events around ``--inner`` back-to-back calls, warm-up first, the forms alternated inside every repetition; medians and the
10 / 90 % quantiles go to ``profiles/plane_timecorr_cost.json``.  The timed samples re-read one state of the fields, which at these
sizes fits the Infinity Cache together with a few bases and no longer does with eight.

    python profiles/plane_timecorr_cost.py [--reps 20] [--inner 10] [--out profiles/plane_timecorr_cost.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import fluidgym_amd  # noqa: E402
from fluidgym_amd.simulation.plane_timecorr import PlaneTimeCorrelation  # noqa: E402

WORKLOADS = (("TCF3D-baseline-v0", 8, ("u", "v", "w")), ("RBC2D-baseline-v0", 32, ("u", "v")))
LIVE = (1, 4, 8)


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


def measure(env_id, envs, channels, reps, inner, triad_gbps):
    env = fluidgym_amd.make(env_id, num_envs=envs, use_marl=False, randomize_initial_state=False, load_domain_statistics=False)
    env.reset(seed=0)
    zero = torch.zeros(env._zero_action.shape, device=env.cuda_device)
    assert env._hook("flow_timecorr") is None                                  # the recorder is off: the step path of the parent commit

    def env_step():
        env._n_steps = 0
        env.step(zero)

    env_step()
    u = env._block.velocity
    recs = {n: PlaneTimeCorrelation(channels, n, 1) for n in LIVE}
    jobs = {"timecorr_%d_slots" % n: (lambda r=recs[n]: r.update(u, time=0.0)) for n in LIVE}
    jobs["sim_step"] = env._sim.single_step
    for _ in range(max(LIVE) + 2):                                      # fills every ring: from here on all slots are live
        for j in jobs.values():
            j()
    for n, r in recs.items():
        assert sum(lag >= 0 for lag in r.slot_lags(r.samples)) == n
    ms = {k: [] for k in jobs}
    step_ms = []
    for r in range(reps):
        for k, j in jobs.items():
            ms[k].append(event_ms(j, inner))
        if r % 5 == 0:
            step_ms.append(event_ms(env_step, 1))
    torch.cuda.synchronize()
    coef = recs[4].coefficient(channels[0])
    assert np.nanmax(np.abs(coef[..., 0] - 1.0)) < 1e-6                # the timed launches computed a correlation
    K, item = len(channels), u.element_size()
    field = u[:, 0].numel() * item
    out = {"envs": envs, "channels": list(channels), "velocity": list(u.shape), "sim_steps_per_env_step": env._n_sim_steps,
           "field_bytes": field, "slot_bytes": K * field, "sim_step": summarise(ms.pop("sim_step")), "env_step": summarise(step_ms)}
    for n in LIVE:
        s = summarise(ms["timecorr_%d_slots" % n])
        s["model_bytes"] = (2 + n) * K * field
        s["model_GB_per_s"] = s["model_bytes"] / s["median_ms"] * 1e-6
        s["fraction_of_triad"] = s["model_GB_per_s"] / triad_gbps
        s["share_of_sim_step"] = s["median_ms"] / out["sim_step"]["median_ms"]
        out["timecorr_%d_slots" % n] = s
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "plane_timecorr_cost.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    torch.cuda.set_device(0)
    triad = bench.stream_triad(torch.device("cuda", 0))
    out = {"device": torch.cuda.get_device_name(0), "stream_triad": triad,
           "clock": f"device events around {args.inner} back-to-back calls (env step: one call), {args.reps} repetitions, the forms alternated",
           "byte_model": "(2 + live slots) * K * field bytes"}
    for env_id, envs, channels in WORKLOADS:
        out[env_id] = measure(env_id, envs, channels, args.reps, args.inner, triad["GBps"])
        print(env_id, json.dumps(out[env_id]), flush=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
