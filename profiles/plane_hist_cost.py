"""What one sample of the plane histograms costs per launch (``fg_plane_histogram``): 8 envs of the 128 x 64 x 64 channel (u, v, w, p;
the workgroup form) and 32 envs of the 512 x 128 RBC2D grid (u, v, p, T; the small-plane form), ``bins = 128``, one pair at
``joint_bins = 32``, every row listed.  Two inputs: normal data spread over the range, and every cell in one bin (all lanes of a
wave on one LDS counter).  Beside them, on the same tensors and the same card: one ``fg_plane_moments`` sample of order 2, and a
device-to-device copy of as many bytes as the histogram kernel reads.  Only kernels are timed: tables and accumulators are allocated
beforehand and the library is called directly.  Device events around runs of ``--launches`` back-to-back launches, warm-up first, the
forms alternated inside every repetition; medians and the 10 / 90 % quantiles per launch go to ``profiles/plane_hist_cost.json``.
There is no bar to meet: the number is a record.

    python profiles/plane_hist_cost.py [--reps 100] [--launches 10] [--out profiles/plane_hist_cost.json]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fluidgym_amd import _lib as L  # noqa: E402

BINS, JOINT_BINS = 128, 32


def summarise(us):
    us = np.asarray(us)
    return {"median_us": float(np.median(us)), "p10_us": float(np.quantile(us, 0.1)), "p90_us": float(np.quantile(us, 0.9)), "n": int(us.size)}


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def workload(name, B, dims, grid, scalar, launches, reps):
    lib, dev = L.load(), torch.device("cuda", 0)
    torch.manual_seed(0)
    nz, ny, nx = ((1,) + grid)[-3:]
    cells = nz * ny * nx
    K = dims + 1 + (1 if scalar else 0)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    rows = (ctypes.c_int32 * ny)(*range(ny))
    pairs = (ctypes.c_int32 * 2)(0, 1)
    lo = torch.full((ny, K), -4.0, dtype=torch.float32, device=dev)
    scale = torch.full((ny, K), BINS / 8.0, dtype=torch.float32, device=dev)
    counts = torch.zeros(B, ny, K, BINS + 3, dtype=torch.int64, device=dev)
    joint = torch.zeros(B, ny, 1, JOINT_BINS * JOINT_BINS + 1, dtype=torch.int64, device=dev)
    n, tickets = torch.zeros(B, dtype=torch.float64, device=dev), torch.zeros(B, dtype=torch.int64, device=dev)
    mean = torch.empty(B, ny, K, dtype=torch.float64, device=dev)
    central = torch.empty(B, ny, K * (K + 1) // 2, dtype=torch.float64, device=dev)
    nbytes = B * K * cells * 4
    src = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)

    def tensors(spread):
        make = (lambda *s: torch.randn(*s, dtype=torch.float32, device=dev)) if spread else \
               (lambda *s: torch.full(s, 0.3, dtype=torch.float32, device=dev))
        fields = [make(B, dims, *grid), make(B, 1, *grid)] + ([make(B, 1, *grid)] if scalar else [])
        parts = [(fields[0], c) for c in range(dims)] + [(f, 0) for f in fields[1:]]
        ptrs = (ctypes.c_void_p * K)(*[t.data_ptr() + c * cells * 4 for t, c in parts])
        strides = (ctypes.c_int64 * K)(*[int(t.shape[1]) * cells for t, _ in parts])
        return fields, ptrs, strides

    data = {"spread": tensors(True), "one_bin": tensors(False)}

    def hist(which):
        _, ptrs, strides = data[which]
        L.check(lib.fg_plane_histogram(ptrs, strides, K, B, nz, ny, nx, rows, ny, ptr(lo), ptr(scale), BINS, pairs, 1, JOINT_BINS,
                                       ptr(counts), ptr(joint), stream))

    def moments():
        _, ptrs, strides = data["spread"]
        L.check(lib.fg_plane_moments(ptrs, strides, K, B, nz, ny, nx, 2, ptr(n), ptr(mean), ptr(central), ptr(tickets), stream))

    jobs = {"histogram_spread": lambda: hist("spread"), "histogram_one_bin": lambda: hist("one_bin"), "moments_order2": moments,
            "copy": lambda: dst.copy_(src)}
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
    res = {k: summarise(v) for k, v in us.items()}
    spread = res["histogram_spread"]["median_us"]
    res.update({"batch": B, "grid_nz_ny_nx": [nz, ny, nx], "K": K, "bins": BINS, "pairs": 1, "joint_bins": JOINT_BINS,
                "form": "one wave per row" if nz * nx <= 1024 else "one workgroup per row", "bytes_read": int(nbytes),
                "ratio_to_moments": spread / res["moments_order2"]["median_us"], "ratio_to_copy": spread / res["copy"]["median_us"],
                "one_bin_over_spread": res["histogram_one_bin"]["median_us"] / spread, "read_GBps": nbytes / spread * 1e-3})
    samples = 5 + reps * launches                # every histogram launch added one sample: the counters must say so
    total = counts.sum(dim=-1)
    assert bool((total == 2 * samples * nz * nx).all()), "the counters do not add up to the cells seen"
    print(name, json.dumps(res))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "plane_hist_cost.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    out = {"device": torch.cuda.get_device_name(0), "dtype": "float32 fields, uint64 counters",
           "clock": f"device events around {args.launches} back-to-back launches, per launch",
           "yardsticks": "fg_plane_moments (order 2) on the same tensors; torch device-to-device copy of bytes_read (read once, written once)"}
    out["tcf_8x128x64x64"] = workload("tcf_8x128x64x64", 8, 3, (128, 64, 64), False, args.launches, args.reps)
    out["rbc2d_32x512x128"] = workload("rbc2d_32x512x128", 32, 2, (128, 512), True, args.launches, args.reps)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
