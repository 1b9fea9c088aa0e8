"""Writes tests/golden/mbc_forms.npz, the fixture of tests/test_gpu_mbc_forms.py: inputs and bit-exact outputs of every launched form
of the chunked multi-block pressure CG.  Needs the GPU; run from the repository root (``python tests/golden/make_golden_mbc_forms.py``)
at the commit whose bits are the yardstick.  Not run by the suite.

Inputs, per mesh: the pressure matrix the fp32 library assembles in one PISO step from a random velocity (P_DIAG / P_OFF read back;
the fp64 library gets the same words widened), a normal right-hand side with its mean removed, different per env, and a positive
unit vector for the general residual projection.  The tolerance of each library is the first of its candidates (around 1e-6 / 1e-12)
at which the long solve of the 1200-cell mesh converges, and only behind the restart at iteration 100, and the preconditioned solve
takes more than 20 iterations.  Outputs: what tests/test_gpu_mbc_forms.py::solve_case returns, per case and iteration cap."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from fluidgym_amd import _lib as L  # noqa: E402
from tests import test_gpu_mbc_forms as T  # noqa: E402

TOLS = {"f32": (1e-6, 2e-6, 5e-7, 4e-6, 2.5e-7, 1e-5), "f64": (1e-12, 1e-11, 1e-13, 1e-10)}


def inputs(mesh, seed):
    rng = np.random.default_rng(seed)
    dom = T.MESHES[mesh]().native(batch=T.B)
    N, d = dom.n_cells, dom.dims
    dom.velocity.copy_(torch.as_tensor(0.2 * rng.standard_normal((T.B, d, N)), dtype=torch.float32))
    dom.piso_step([0.05, 0.03], advection_tol=1e-7, pressure_tol=2e-6, pressure_project_mean=True, raise_on_failure=False)
    diag = dom.buffer(L.FG_MB_BUF_P_DIAG).view(T.B, N).cpu().numpy().copy()
    off = dom.buffer(L.FG_MB_BUF_P_OFF).view(T.B, 2 * d, N).cpu().numpy().copy()
    dom.close()
    assert np.isfinite(diag).all() and np.isfinite(off).all() and (diag != 0).all()
    rhs = rng.standard_normal((T.B, N))
    rhs = (rhs - rhs.mean(1, keepdims=True)).astype(np.float32)
    yp = rng.uniform(0.5, 1.5, N)
    yp = (yp / np.linalg.norm(yp)).astype(np.float32)
    return {"diag": diag, "off": off, "rhs": rhs, "yp": yp}


def main(path):
    for k, v in T.SWITCHES.items():
        os.environ[k] = v
    out, inp = {}, {}
    for seed, mesh in enumerate(T.MESHES):
        inp[mesh] = inputs(mesh, 200 + seed)
        for k, v in inp[mesh].items():
            out[f"{mesh}.{k}"] = v
        print(mesh, "cells", inp[mesh]["diag"].shape[1], "diag", float(inp[mesh]["diag"].min()), float(inp[mesh]["diag"].max()), flush=True)

    def solve(lib, mesh, pre, pm, tol):
        i = inp[mesh]
        return T.solve_case(lib, mesh, pre, pm, i["diag"], i["off"], i["rhs"], i["yp"], tol)

    first = {}   # the solves behind the chosen tolerances: the recorded ones must repeat them bit for bit
    for lib, cands in TOLS.items():
        chosen = None
        for tol in cands:
            runs = {(lib, "channel40x30", False, 1): solve(lib, "channel40x30", False, 1, tol)}
            runs.update({(lib, "polar_ring", True, pm): solve(lib, "polar_ring", True, pm, tol) for pm in (0, 1)})
            long_, pres = runs[(lib, "channel40x30", False, 1)][-1], [runs[(lib, "polar_ring", True, pm)][-1] for pm in (0, 1)]
            ok = bool(long_["converged"].all() and (long_["iterations"] > 100).all() and all((p["iterations"] > 20).all() for p in pres))
            print(lib, "tol", tol, "channel40x30 pm1: iterations", long_["iterations"].tolist(), "converged", long_["converged"].tolist(),
                  "| polar_ring preconditioned pm0 / pm1: iterations", [p["iterations"].tolist() for p in pres],
                  "converged", [p["converged"].tolist() for p in pres], "->", "ok" if ok else "no", flush=True)
            if ok:
                chosen = tol
                first.update(runs)
                break
        assert chosen is not None, f"no tolerance of {cands} meets the conditions in the {lib} library"
        out["tol." + lib] = np.float64(chosen)

    for lib, mesh, pre, pm in T.CASES:
        res = solve(lib, mesh, pre, pm, float(out["tol." + lib]))
        for r, r0 in zip(res, first.get((lib, mesh, pre, pm), res)):
            assert np.array_equal(r["work"], r0["work"]), "a solve did not repeat its bits"
        key = T.case_key(lib, mesh, pre, pm)
        for name in ("work", "iterations", "converged", "residual"):
            out[f"{key}.{name}"] = np.stack([r[name] for r in res])
        print(key, "iterations", [r["iterations"].tolist() for r in res], "converged", [r["converged"].tolist() for r in res],
              "residual", [["%.3e" % v for v in r["residual"]] for r in res], flush=True)
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(path, size, "bytes")
    assert size < 1 << 20


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN)
