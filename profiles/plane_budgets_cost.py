"""What one sample of the Reynolds-stress budgets costs at the TCF shape (8 envs, velocity ``[8, 3, 64, 64, 128]``, fp32): one
``PlaneBudgets.update`` without and with forcing (one launch of ``fg_plane_budgets``), beside the torch expression of the reference's
``update_from_data`` on the same tensors (twelve padded central differences, a mean, a full-field difference and a sum per moment,
the merges) and beside a plain read of the four fields (``torch.sum`` of velocity and of pressure).  Device events around
``--inner`` back-to-back calls, warm-up first, the forms alternated inside every repetition; medians and the 10 / 90 % quantiles
go to ``profiles/plane_budgets_cost.json``.  The timed calls re-read the same fields, which fit the Infinity Cache.

    python profiles/plane_budgets_cost.py [--reps 30] [--inner 10] [--out profiles/plane_budgets_cost.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fluidgym_amd.simulation.plane_budgets import PlaneBudgets, budget_keys  # noqa: E402


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


class TorchBudgets:
    """The arithmetic of the reference's accumulation in torch, batched over the envs: zero-padded central differences over the
    coordinate distances, per moment a product of deviations and a sum over (z, x), the pairwise merge."""

    def __init__(self, x, y, z, device, dtype):
        self.keys = budget_keys(False)
        self.index = {k: q for q, k in enumerate(self.keys)}
        self.rdist = []
        for pos, dim in ((x, 3), (y, 2), (z, 1)):
            g = np.concatenate([[2 * pos[0] - pos[1]], pos, [2 * pos[-1] - pos[-2]]])
            shape = [1, 1, 1, 1]
            shape[dim] = -1
            self.rdist.append((dim, torch.as_tensor(1.0 / np.abs(g[2:] - g[:-2]), device=device, dtype=dtype).reshape(shape)))
        self.n, self.mean, self.cen = 0, None, None

    def grad(self, f, axis):
        dim, r = self.rdist[axis]
        pad = [0, 0, 0, 0, 0, 0]
        pad[2 * (3 - dim)] = pad[2 * (3 - dim) + 1] = 1
        g = torch.nn.functional.pad(f, pad)
        return (g.narrow(dim, 2, f.shape[dim]) - g.narrow(dim, 0, f.shape[dim])) * r

    def update(self, u, p):
        f = [u[:, 0], u[:, 1], u[:, 2]]
        ch = f + [self.grad(p[:, 0], a) for a in range(3)] + [self.grad(f[i], a) for a in range(3) for i in range(3)]
        n1 = u.shape[2] * u.shape[4]
        mean = [torch.mean(c, dim=(1, 3), keepdim=True) for c in ch]
        d = [c - m for c, m in zip(ch, mean)]
        cen = []
        for key in self.keys:
            m = d[key[0]] * d[key[1]]
            if len(key) == 3:
                m = m * d[key[2]]
            cen.append(torch.sum(m, dim=(1, 3)))
        mean = [m[:, 0, :, 0] for m in mean]
        if self.mean is not None:
            n0, n = self.n, self.n + n1
            dl = [b - a for a, b in zip(self.mean, mean)]
            merged = []
            for q, key in enumerate(self.keys):
                if len(key) == 2:
                    merged.append(self.cen[q] + cen[q] + dl[key[0]] * dl[key[1]] * (n0 * n1 / n))
                else:
                    i, j, k = key
                    cross = sum(dl[a] * (n0 * cen[self.index[pr]] - n1 * self.cen[self.index[pr]]) for a, pr in ((i, (j, k)), (j, (i, k)), (k, (i, j))))
                    merged.append(self.cen[q] + cen[q] + dl[i] * dl[j] * dl[k] * (n0 * n1 * (n0 - n1) / (n * n)) + cross / n)
            mean = [(n0 * a + n1 * b) / n for a, b in zip(self.mean, mean)]
            cen = merged
        self.n, self.mean, self.cen = self.n + n1, mean, cen


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--shape", type=int, nargs=4, default=[8, 64, 64, 128], metavar=("B", "NZ", "NY", "NX"))
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "plane_budgets_cost.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    B, nz, ny, nx = args.shape
    gen = torch.Generator(device="cuda").manual_seed(0)
    e = np.tanh(2.0 * np.linspace(-1, 1, ny + 1)) / np.tanh(2.0)
    x, y, z = (np.arange(nx) + 0.5) * (2 * np.pi / nx), 0.5 * (e[1:] + e[:-1]), (np.arange(nz) + 0.5) * (np.pi / nz)
    prof = torch.as_tensor(1.0 - y ** 2, device="cuda", dtype=torch.float32).view(1, 1, 1, ny, 1)
    u = 0.1 * torch.randn(B, 3, nz, ny, nx, device="cuda", generator=gen)
    u[:, :1] += prof
    p = 0.05 * torch.randn(B, 1, nz, ny, nx, device="cuda", generator=gen)
    s = torch.zeros_like(u)
    s[:, 0] = 1.0
    # the torch form zero-pads every axis, as the reference does: the kernel is timed in the same border mode
    plain, forced = PlaneBudgets(x, y, z, wrap=(False, False)), PlaneBudgets(x, y, z, forcing=True, wrap=(False, False))
    ref = TorchBudgets(x, y, z, u.device, u.dtype)
    jobs = {"plane_budgets": lambda: plain.update(u, p), "plane_budgets_forcing": lambda: forced.update(u, p, s),
            "torch_budgets": lambda: ref.update(u, p), "read_four_fields": lambda: (torch.sum(u), torch.sum(p))}
    for _ in range(3):
        for j in jobs.values():
            j()
    # the two agree on what they computed (fp32 torch against the fp64 kernel)
    q = ref.index[(9, 9)]
    got, want = plain.central_sum((9, 9)), ref.cen[q].double().cpu().numpy()
    assert np.allclose(got, want, rtol=1e-3), float(np.abs(got / want - 1).max())
    ms = {k: [] for k in jobs}
    for _ in range(args.reps):
        for k, j in jobs.items():
            ms[k].append(event_ms(j, args.inner))
    item = u.element_size()
    out = {"shape": {"velocity": list(u.shape), "pressure": list(p.shape)}, "device": torch.cuda.get_device_name(0),
           "algorithmic_bytes": 4 * p.numel() * item,
           "clock": f"device events around {args.inner} back-to-back calls, {args.reps} repetitions, the forms alternated"}
    out.update({k: summarise(v) for k, v in ms.items()})
    for k in ("plane_budgets", "plane_budgets_forcing"):
        out[k]["over_plain_read"] = out[k]["median_ms"] / out["read_four_fields"]["median_ms"]
    out["torch_over_kernel"] = out["torch_budgets"]["median_ms"] / out["plane_budgets"]["median_ms"]
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
