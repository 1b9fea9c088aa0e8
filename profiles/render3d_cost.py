"""What one launch of the ray marcher costs (``fg_render_isosurface`` / ``fg_render_volume``) at
``size=(480, 640)``: 8 envs of the small channel's render grid (128 x 81 x 64, the iso-surface of one channel coloured by the norm of
three, the family's clip box and view) and 64 envs of the 3-D cylinder's render grid at the default resolution (515 x 96 x 96, the
iso-surface of the norm of three channels coloured by the norm of three, the cylinder as solid body, the family's clip box and view),
each also in volume mode and with a level no sample reaches (every ray marches through the whole box and hits nothing: what the empty
space costs, the evidence a brick-skipping change would rest on).  Yardsticks on the same card: ``frames.colorize`` of one plane of
the same view, and a device-to-device copy of one channel of the volume.  The fields are smooth noise (a coarse random grid,
interpolated), scaled so that the level cuts them.  Only the kernels are timed: tables, ranges, levels and results are allocated
beforehand and the library is called directly.  Device events around ``--launches`` back-to-back launches of the ray marcher and
``--short-launches`` of the two yardsticks (one launch of those takes some 10 us, which is the timer's floor and not the kernel),
warm-up first, the forms alternated inside every repetition; medians and the 10 / 90 % quantiles per launch go to
``profiles/render3d_cost.json``.  There is no bar to meet: the number is a record.

What the empty space costs is counted, not inferred: from the depth the surface launch wrote, ``ray_samples`` restates how many samples
every ray took before it stopped (a ray needs the two that bracket its hit; every other one fell into empty space), per ray and per
wave (a wave of 8 x 8 rays marches until its last ray stops), and the record holds the share of the samples that were empty beside the
time per wave step of the surface launch and of the launch that hits nothing.

    python profiles/render3d_cost.py [--reps 10] [--launches 1] [--short-launches 200] [--out profiles/render3d_cost.json]
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
from fluidgym_amd.envs import frames as F  # noqa: E402
from fluidgym_amd.envs import render3d as R3  # noqa: E402

SIZE = (480, 640)


def summarise(us):
    us = np.asarray(us)
    return {"median_us": float(np.median(us)), "p10_us": float(np.quantile(us, 0.1)), "p90_us": float(np.quantile(us, 0.9)), "n": int(us.size)}


def smooth_noise(shape, dev, seed):
    """``[B, C, nz, ny, nx]``: a coarse random grid interpolated to the shape, about unit variance."""
    g = torch.Generator(device=dev).manual_seed(seed)
    B, C, nz, ny, nx = shape
    coarse = torch.randn((B, C, max(nz // 8, 2), max(ny // 8, 2), max(nx // 8, 2)), device=dev, generator=g)
    return torch.nn.functional.interpolate(coarse, size=(nz, ny, nx), mode="trilinear", align_corners=True).contiguous()


def ray_samples(cam, shape3, step, depth):
    """Samples taken per ray ``[B, H, W]`` (float64; 0 for a ray that misses the box) and samples a ray that hits nothing takes
    ``[H, W]``, from the slabs of the kernel's written order and the depth a launch wrote."""
    nz, ny, nx = shape3
    B, H, W = depth.shape
    c = torch.from_numpy(R3.camera_array(cam).astype(np.float64)).to(depth.device)
    pj = (torch.arange(W, device=depth.device, dtype=torch.float64) + 0.5)[None, :, None]
    pi = (torch.arange(H, device=depth.device, dtype=torch.float64) + 0.5)[:, None, None]
    o, d = c[0] + pj * c[1] + pi * c[2], c[3] + pj * c[4] + pi * c[5]
    tmin = torch.zeros((H, W), dtype=torch.float64, device=depth.device)
    tmax = torch.full((H, W), float("inf"), dtype=torch.float64, device=depth.device)
    miss = torch.zeros((H, W), dtype=torch.bool, device=depth.device)
    for a, n in enumerate((nx, ny, nz)):
        oa, da = o[..., a], d[..., a]
        par = da == 0
        safe = torch.where(par, torch.ones_like(da), da)
        t1, t2 = (0.0 - oa) / safe, (float(n - 1) - oa) / safe
        miss |= par & ((oa < 0) | (oa > n - 1))
        tmin = torch.where(par, tmin, torch.maximum(tmin, torch.minimum(t1, t2)))
        tmax = torch.where(par, tmax, torch.minimum(tmax, torch.maximum(t1, t2)))
    miss |= ~(tmin <= tmax)
    whole = torch.where(miss, torch.zeros_like(tmin), torch.floor((tmax - tmin) / step).clamp(max=65535.0) + 1.0)
    hit = torch.isfinite(depth)
    to_hit = torch.minimum(torch.floor((depth.double() - tmin) / step) + 2.0, whole.expand_as(depth))
    return torch.where(hit, to_hit, whole.expand_as(depth)), whole


def empty_space(cam, shape3, step, depth):
    """The counts of the docstring: samples and wave steps (the largest count of each 8 x 8 patch), taken and needed."""
    taken, whole = ray_samples(cam, shape3, step, depth)
    B, H, W = depth.shape
    hit = torch.isfinite(depth)
    patches = lambda t: t.reshape(t.shape[0], H // 8, 8, W // 8, 8)
    wave_taken = patches(taken).amax(dim=(2, 4)).sum().item()
    wave_whole = patches(whole[None]).amax(dim=(2, 4)).sum().item() * B
    wave_needed = 2.0 * patches(hit).any(dim=4).any(dim=2).sum().item()
    samples, needed = taken.sum().item(), 2.0 * hit.sum().item()
    return {"samples_taken": samples, "samples_per_ray": samples / (B * H * W), "empty_sample_share": 1.0 - needed / samples,
            "wave_steps_taken": wave_taken, "empty_wave_step_share": 1.0 - wave_needed / wave_taken,
            "wave_steps_level_out_of_reach": wave_whole}


def workload(name, B, shape3, channel, level, clip, solid, extent, elev, azim, launches, short_launches, reps):
    lib, dev = L.load(), torch.device("cuda", 0)
    nz, ny, nx = shape3
    H, W = SIZE
    vol = smooth_noise((B, 3, nz, ny, nx), dev, 0)
    cvol = smooth_noise((B, 3, nz, ny, nx), dev, 1)
    table = F.device_table("rainbow", dev)
    opacity = torch.from_numpy(R3.log_opacity_table(0.05)).to(dev)
    rng = torch.tensor([[0.0, 2.0]] * B, dtype=torch.float32, device=dev)
    vrng = torch.tensor([[-2.0, 4.0]] * B, dtype=torch.float32, device=dev)
    levels = {"surface": torch.full((B,), level, dtype=torch.float32, device=dev), "empty": torch.full((B,), 1e6, dtype=torch.float32, device=dev)}
    envs = np.arange(B, dtype=np.int32)
    env_p = envs.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    cam = R3.orbit_camera(shape3, extent, elev, azim, size=SIZE)
    opt = R3._options(None, cam, clip, R3.BODY_COLOR, (255, 255, 255))
    out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev)
    depth = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    plane_spec = F.FrameSpec(channel=channel, axis=0, index=nz // 2).c_struct()
    plane = torch.empty((B, ny, nx, 3), dtype=torch.uint8, device=dev)
    copy_dst = torch.empty((B, nz, ny, nx), dtype=torch.float32, device=dev)

    def iso(which, with_solid=True):
        L.check(lib.fg_render_isosurface(p(vol), B, 3, nz, ny, nx, channel, p(levels[which]), p(cvol), 3, -1, p(rng), p(table),
                                         p(solid) if with_solid else None, ctypes.byref(cam), ctypes.byref(opt), H, W, env_p, B, p(out),
                                         p(depth), stream))

    def volume():
        L.check(lib.fg_render_volume(p(vol), B, 3, nz, ny, nx, 0, p(vrng), p(table), p(opacity), ctypes.byref(cam), ctypes.byref(opt), H, W,
                                     env_p, B, p(out), stream))

    def colorize():
        L.check(lib.fg_frame_colorize(p(vol), B, 3, nz, ny, nx, ctypes.byref(plane_spec), p(table), None, p(rng), env_p, B, p(plane), stream))

    jobs = {"isosurface": lambda: iso("surface"), "isosurface_level_out_of_reach": lambda: iso("empty"), "volume": volume,
            "colorize_one_plane": colorize, "copy_one_channel": lambda: copy_dst.copy_(vol[:, 0])}
    for _ in range(2):
        for j in jobs.values():
            j()
    iso("surface")
    torch.cuda.synchronize()
    no_hit = float(torch.isinf(depth).float().mean().item())
    assert H % 8 == 0 and W % 8 == 0
    empty = empty_space(cam, shape3, float(opt.step), depth)
    count = {k: (short_launches if k in ("colorize_one_plane", "copy_one_channel") else launches) for k in jobs}
    us = {k: [] for k in jobs}
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(reps):
        for k, j in jobs.items():               # the forms alternate inside every repetition
            start.record()
            for _ in range(count[k]):
                j()
            stop.record()
            stop.synchronize()
            us[k].append(1e3 * start.elapsed_time(stop) / count[k])
    res = {"volume_shape": [B, 3, nz, ny, nx], "frame_shape": [B, H, W, 3], "iso_channel": channel, "solid_body": solid is not None,
           "step": float(opt.step), "pixels_without_a_hit": no_hit, "volume_bytes_one_channel": int(B * nz * ny * nx * 4)}
    res.update({k: dict(summarise(v), launches_per_timing=count[k]) for k, v in us.items()})
    res.update(empty)
    t = {k: res[k]["median_us"] for k in jobs}
    res["us_per_frame_isosurface"] = t["isosurface"] / B
    res["empty_march_over_isosurface"] = t["isosurface_level_out_of_reach"] / t["isosurface"]
    res["ns_per_wave_step_isosurface"] = 1e3 * t["isosurface"] / empty["wave_steps_taken"]
    res["ns_per_wave_step_level_out_of_reach"] = 1e3 * t["isosurface_level_out_of_reach"] / empty["wave_steps_level_out_of_reach"]
    print(name, json.dumps(res))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--launches", type=int, default=1)
    ap.add_argument("--short-launches", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "render3d_cost.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda", 0)
    out = {"device": torch.cuda.get_device_name(0), "dtype": "float32 in, uint8 RGB out", "size": list(SIZE),
           "clock": f"device events around {args.launches} back-to-back launches ({args.short_launches} of the yardsticks), per launch",
           "yardsticks": "fg_frame_colorize of the mid z plane of the same view; torch device-to-device copy of one channel of the volume"}
    nz, ny, nx = 64, 81, 128                 # render_shape (128, 81, 64) of the small channel
    out["tcf_render_128x81x64_B8"] = workload("tcf_render_128x81x64_B8", 8, (nz, ny, nx), 0, 1.0, ((0, 0, 0), (nx - 1, 33, nz - 1)), None,
                                              (np.pi, 2.0, np.pi / 2), 15, 60, args.launches, args.short_launches, args.reps)
    nz, ny, nx = 96, 96, 515                 # render_shape (515, 96, 96) of the 3-D cylinder at resolution 24
    zz, yy, xx = torch.meshgrid(torch.arange(nz, device=dev), torch.arange(ny, device=dev), torch.arange(nx, device=dev), indexing="ij")
    solid = (((xx - 47) ** 2 + (yy - 46) ** 2) <= 11 ** 2).to(torch.uint8).contiguous()
    out["cylinder_render_515x96x96_B64"] = workload("cylinder_render_515x96x96_B64", 64, (nz, ny, nx), -1, 2.0,
                                                    ((20, 15, 0), (nx - 1, ny - 16, nz - 1)), solid, (22.0, 4.1, 4.1), 10, 60,
                                                    args.launches, args.short_launches, args.reps)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
