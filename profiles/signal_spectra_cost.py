"""What one sample of the signal spectra costs: one ``SignalSpectra.update`` (one launch of ``fg_signal_spectra``) on a batch of 64
envs with 4 signals and 2 pairs, fp32, for ``segment`` = 64, 256 and 1024 -- once with no segment due in any env (the append alone:
what all but one in ``hop`` samples cost) and once with a segment due in every env (``noverlap = segment - 1`` on a full ring: 4 + 2
jobs per env) -- beside one sim step of ``CylinderJet2D-easy-v0`` x 64 with the recorder off, the yardstick.  Device events around
``--inner`` back-to-back calls, warm-up first, the forms alternated inside every repetition; medians and the 10 / 90 % quantiles go
to ``profiles/signal_spectra_cost.json``.

    python profiles/signal_spectra_cost.py [--reps 20] [--inner 20] [--out profiles/signal_spectra_cost.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fluidgym_amd  # noqa: E402
from fluidgym_amd.simulation.signal_spectra import SignalSpectra  # noqa: E402

ENVS, NAMES, PAIRS = 64, ("drag", "lift", "u@0", "p@0"), (("lift", "u@0"), ("lift", "p@0"))
SEGMENTS = (64, 256, 1024)


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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "signal_spectra_cost.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    torch.cuda.set_device(0)
    env = fluidgym_amd.make("CylinderJet2D-easy-v0", num_envs=ENVS, randomize_initial_state=False)
    env.reset(seed=0)
    assert env.signal_spectra is None                                         # the recorder is off: the step path as it was
    forces = torch.randn(ENVS, 2, device="cuda")
    probes = torch.randn(ENVS, 2, device="cuda")
    jobs = {"sim_step": env._sim.single_step}
    recs = {}
    for L in SEGMENTS:
        # never due while timed: the counter is put back behind a fresh start before every repetition (inner < L)
        idle = SignalSpectra(NAMES, L, 0, "hann", "constant", PAIRS)
        due = SignalSpectra(NAMES, L, L - 1, "hann", "constant", PAIRS)
        for _ in range(L):
            due.update(forces, probes)                                        # a full ring: from here on every sample is due
        idle.update(forces, probes)
        recs[L] = (idle, due)
        assert args.inner < L
        jobs[f"append_{L}"] = lambda r=idle: r.update(forces, probes)
        jobs[f"segment_{L}"] = lambda r=due: r.update(forces, probes)
    for j in jobs.values():
        j()
    ms = {k: [] for k in jobs}
    for _ in range(args.reps):
        for k, j in jobs.items():
            if k.startswith("append_"):
                recs[int(k.split("_")[1])][0].restart()
            ms[k].append(event_ms(j, args.inner))
    torch.cuda.synchronize()
    out = {"device": torch.cuda.get_device_name(0), "envs": ENVS, "signals": len(NAMES), "pairs": len(PAIRS),
           "clock": f"device events around {args.inner} back-to-back calls, {args.reps} repetitions, the forms alternated",
           "sim_step": summarise(ms.pop("sim_step"))}
    for L in SEGMENTS:
        idle, due = recs[L]
        assert idle.segments.tolist() == [0] * ENVS and int(due.segments.min()) > args.reps * args.inner
        for k in (f"append_{L}", f"segment_{L}"):
            out[k] = summarise(ms[k])
            out[k]["share_of_sim_step"] = out[k]["median_ms"] / out["sim_step"]["median_ms"]
    env.close()
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
