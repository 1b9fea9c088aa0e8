"""What drawing the frames of a batch costs per launch (``fg_frame_colorize``): 64 envs of the 256 x 128 channel (the speed: two
channels read per pixel) and 64 envs of the cylinder's render grid at the default resolution (515 x 96, one channel, the cylinder
mask), each beside a device-to-device copy that moves the same algorithmic bytes (field read + mask read + frames written; the copy
reads half of them and writes half) on the same card.  Only the kernel is timed: the range tensor, the table and the result are
allocated beforehand and the library is called directly.  Device events around runs of ``--launches`` back-to-back launches, warm-up
first, the forms alternated inside every repetition; medians and the 10 / 90 % quantiles per launch are written to
``profiles/frames_cost.json``.  There is no bar to meet: the number is a record.

    python profiles/frames_cost.py [--reps 100] [--launches 10] [--out profiles/frames_cost.json]
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
from fluidgym_amd.envs.frames import FrameSpec, device_table  # noqa: E402


def summarise(us):
    us = np.asarray(us)
    return {"median_us": float(np.median(us)), "p10_us": float(np.quantile(us, 0.1)), "p90_us": float(np.quantile(us, 0.9)), "n": int(us.size)}


def workload(name, shape, spec, value_range, masked, launches, reps):
    lib, dev = L.load(), torch.device("cuda", 0)
    torch.manual_seed(0)
    B, C, nz, ny, nx = shape
    field = torch.randn(shape, dtype=torch.float32, device=dev)
    H, W = spec.frame_shape(nz, ny, nx)
    mask = None
    if masked:
        yy, xx = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
        mask = (((yy - H // 2) ** 2 + (xx - W // 10) ** 2) <= (H // 8) ** 2).to(torch.uint8).contiguous()
    table = device_table("viridis", dev)
    rng = torch.tensor([[value_range[0], value_range[1] - value_range[0]]] * B, dtype=torch.float32, device=dev)
    envs = np.arange(B, dtype=np.int32)
    out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev)
    c_spec = spec.c_struct()
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    read_channels = C if spec.channel < 0 else 1
    nbytes = B * H * W * (4 * read_channels + 3 + (1 if masked else 0))
    src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)

    def draw():
        L.check(lib.fg_frame_colorize(ctypes.c_void_p(field.data_ptr()), B, C, nz, ny, nx, ctypes.byref(c_spec), ctypes.c_void_p(table.data_ptr()),
                                      ctypes.c_void_p(mask.data_ptr()) if masked else None, ctypes.c_void_p(rng.data_ptr()),
                                      envs.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), B, ctypes.c_void_p(out.data_ptr()), stream))

    jobs = {"kernel": draw, "copy": lambda: dst.copy_(src)}
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
    k, c = summarise(us["kernel"]), summarise(us["copy"])
    res = {"field_shape": list(shape), "frame_shape": [B, H, W, 3], "channels_read": read_channels, "masked": bool(masked),
           "algorithmic_bytes": int(nbytes), "field_bytes": int(field.numel() * 4), "kernel": k, "copy": c,
           "ratio_to_copy": k["median_us"] / c["median_us"], "algorithmic_GBps": nbytes / k["median_us"] * 1e-3}
    print(name, json.dumps(res))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "frames_cost.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    out = {"device": torch.cuda.get_device_name(0), "dtype": "float32 in, uint8 RGB out",
           "clock": f"device events around {args.launches} back-to-back launches, per launch",
           "yardstick": "torch device-to-device copy of algorithmic_bytes / 2 (read + written = algorithmic_bytes)"}
    out["channel_256x128_B64_speed"] = workload("channel_256x128_B64_speed", (64, 2, 1, 128, 256), FrameSpec(channel=-1), (0.0, 3.0), False,
                                                args.launches, args.reps)
    out["cylinder_render_515x96_B64_vorticity"] = workload("cylinder_render_515x96_B64_vorticity", (64, 1, 1, 96, 515), FrameSpec(channel=0),
                                                           (-3.0, 3.0), True, args.launches, args.reps)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
