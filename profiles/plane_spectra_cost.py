"""What one sample of the plane spectra costs at the TCF shape (8 envs of 128 x 64 x 64 cells, ``u, v, w, p``, four planes and their
mirror images): one ``PlaneSpectra.update`` (one launch of ``fg_plane_spectra``), beside the torch expression of the reference's
``PSDOnline_Torch.update_from_data`` on the same tensors (``index_select``, ``fftn``, ``abs``, slice, mean over the batch, running
mean; once for the planes and once for their mirrors), and beside one sim step of the same env.  Device events around ``--inner``
back-to-back calls, warm-up first, the forms alternated inside every repetition; medians and the 10 / 90 % quantiles go to
``profiles/plane_spectra_cost.json``.  The timed calls re-read the same fields, which fit the Infinity Cache.

    python profiles/plane_spectra_cost.py [--reps 30] [--inner 10] [--out profiles/plane_spectra_cost.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fluidgym_amd  # noqa: E402
from fluidgym_amd.simulation.plane_spectra import PlaneSpectra, lds_bytes  # noqa: E402
from plane_stats_cost import event_ms, host_ms, summarise  # noqa: E402


class TorchPSD:
    """The arithmetic of ``PSDOnline_Torch`` (planes along dim 3, transform over dims 2 and 4, mean over the batch, symmetric)."""

    def __init__(self, planes, ny, device):
        self.planes = torch.tensor(planes, device=device, dtype=torch.int64)
        self.mirror = ny - self.planes - 1
        self.n, self.fft = 0, 0

    def _one(self, data):
        data = torch.abs(torch.fft.fftn(data, dim=(2, 4)))
        data = data[:, :, :(data.shape[2] + 1) // 2, :, :(data.shape[4] + 1) // 2]
        n_b = data.shape[0]
        data = torch.mean(data, dim=0)
        n = self.n + n_b
        self.fft = (self.fft * self.n + data * n_b) / n
        self.n = n

    def update(self, fields):
        self._one(fields.index_select(3, self.planes))
        self._one(fields.index_select(3, self.mirror))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--envs", type=int, default=8)
    ap.add_argument("--env-id", default="TCF3D-baseline-v0")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "plane_spectra_cost.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    env = fluidgym_amd.make(args.env_id, num_envs=args.envs, use_marl=False, randomize_initial_state=False, load_domain_statistics=False)
    env.reset(seed=0)
    env._n_steps = 0
    env.step(torch.zeros(env._zero_action.shape, device=env.cuda_device))
    u, p = env._block.velocity, env._block.pressure
    B, _, nz, ny, nx = u.shape
    planes = [2, 8, 16, ny // 2 - 1]
    acc = PlaneSpectra(("u", "v", "w", "p"), planes, True)
    ref = TorchPSD(planes, ny, u.device)
    # the reference transforms the velocity alone; here the pressure rides along, so the torch form gets all four channels as well:
    # the concatenation is made once, outside the timed region (in favour of the torch form)
    fields = torch.cat([u, p], dim=1)
    jobs = {"plane_spectra": lambda: acc.update(u, p), "torch_psd": lambda: ref.update(fields)}
    for _ in range(5):
        for j in jobs.values():
            j()
    got, want = acc.pooled().amplitude("u")[0], ref.fft[0].double().cpu().numpy().transpose(1, 0, 2)
    assert np.allclose(got, want, rtol=2e-3, atol=1e-4 * want.max()), float(np.abs(got - want).max() / want.max())
    ms = {k: [] for k in jobs}
    sim_ms = []
    for r in range(args.reps):
        for k, j in jobs.items():
            ms[k].append(event_ms(j, args.inner))
        if r % 3 == 0:
            sim_ms.append(host_ms(env._sim.single_step))
    K, T, item = 4, 2 * len(planes), u.element_size()
    plane_bytes = B * K * T * nz * nx * item
    acc_bytes = 2 * 2 * B * K * T * (nz // 2) * (nx // 2) * 8
    out = {"shape": {"envs": B, "velocity": list(u.shape), "pressure": list(p.shape), "planes": planes, "symmetric": True},
           "device": torch.cuda.get_device_name(0),
           "algorithmic_bytes": {"planes_read_once": plane_bytes, "accumulators_read_and_written_once": acc_bytes, "total": plane_bytes + acc_bytes},
           "lds_bytes_per_workgroup": lds_bytes(nz, nx, item), "workgroups": B * K * T,
           "clock": f"device events around {args.inner} back-to-back calls (inputs and accumulators stay in the Infinity Cache); sim step: "
                    "host clock around work ending in a synchronise",
           "sim_step": summarise(sim_ms)}
    out.update({k: summarise(v) for k, v in ms.items()})
    out["plane_spectra"]["algorithmic_GB_per_s"] = (plane_bytes + acc_bytes) / out["plane_spectra"]["median_ms"] * 1e-6
    out["plane_spectra"]["share_of_sim_step"] = out["plane_spectra"]["median_ms"] / out["sim_step"]["median_ms"]
    out["torch_over_kernel"] = out["torch_psd"]["median_ms"] / out["plane_spectra"]["median_ms"]
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
