"""Writes tests/golden/mbb_forms.npz, the fixture of tests/test_gpu_mbb_forms.py: inputs and bit-exact outputs of every kernel form
of the multi-block BiCGStab.  Needs the GPU; run from the repository root (``python tests/golden/make_golden_mbb_forms.py``) at
the commit whose bits are the yardstick.  Not run by the suite.

Inputs: per mesh, velocity systems on the mesh's neighbour table -- random off-diagonals in [-1, -0.1] (not symmetric), a diagonal
3 % above the row sums (strictly dominant, a few dozen iterations to 1e-6), a normal right-hand side, different per env.  Outputs:
x, the accumulator words, alpha / omega and the outcome counts of fg_mb_debug_bicgstab per form and iteration cap; equal x arrays
are stored once (x_pool, x_index)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from tests import helpers_mb as H  # noqa: E402
from tests import test_gpu_mbb_forms as T  # noqa: E402


def systems(dom, seed):
    rng = np.random.default_rng(seed)
    nbr = dom.neighbors()
    F, N = nbr.shape
    Coff = np.where(nbr[None] >= 0, -rng.uniform(0.1, 1.0, (T.B, F, N)), 0.0)
    A = 1.03 * np.abs(Coff).sum(1) + 0.02
    rhs = rng.standard_normal((T.B, dom.dims, N))
    return A.astype(np.float32), Coff.astype(np.float32), rhs.astype(np.float32)


def main(path):
    out = {}
    for seed, mesh in enumerate(T.MESHES):
        dom = T.MESHES[mesh]().native(batch=T.B)
        A, Coff, rhs = systems(dom, 100 + seed)
        dom.close()
        out[mesh + ".A"], out[mesh + ".Coff"], out[mesh + ".rhs"] = A, Coff, rhs
        pool, index, accs, scs, out4s = [], [], [], [], []
        for vec4, fuse in T.FORMS:
            os.environ["FG_MB_BICG_VEC4"], os.environ["FG_MB_BICG_FUSE"] = str(vec4), str(fuse)
            res = T.solve_form(mesh, A, Coff, rhs)
            row = []
            for x, _, _, _ in res:
                k = next((k for k, y in enumerate(pool) if np.array_equal(T._bits(x), T._bits(y))), len(pool))
                if k == len(pool):
                    pool.append(x)
                row.append(k)
            index.append(row)
            accs.append([r[1] for r in res]); scs.append([r[2] for r in res]); out4s.append([r[3] for r in res])
            print(mesh, "vec4", vec4, "fuse", fuse, "x", row, "out4", [r[3].tolist() for r in res], flush=True)
        del os.environ["FG_MB_BICG_VEC4"], os.environ["FG_MB_BICG_FUSE"]
        out[mesh + ".x_pool"], out[mesh + ".x_index"] = np.stack(pool), np.array(index, np.int32)
        out[mesh + ".acc"], out[mesh + ".sc"], out[mesh + ".out4"] = np.array(accs), np.array(scs), np.array(out4s)
    d = H.polar_ring().oracle()
    rng = np.random.default_rng(10)
    u0 = (0.2 * rng.standard_normal((T.B, d.d, d.N))).astype(np.float32)
    p0 = 0.1 * rng.standard_normal((T.B, d.N))
    p0 = (p0 - p0.mean(1, keepdims=True)).astype(np.float32)
    out["ml.u0"], out["ml.p0"] = u0, p0
    us, ps = [], []
    for ml_fuse in T.ML_FUSE:
        os.environ["FG_MB_ML_FUSE"] = str(ml_fuse)
        steps = [T.multilevel_step(bicg, u0, p0) for bicg in T.ML_BICG]
        us.append([s[0] for s in steps]); ps.append([s[1] for s in steps])
    del os.environ["FG_MB_ML_FUSE"]
    out["ml.u"], out["ml.p"] = np.array(us), np.array(ps)
    print("ml: fused == unfused bits:", [bool(np.array_equal(T._bits(out["ml.u"][0, j]), T._bits(out["ml.u"][1, j]))) for j in range(2)], flush=True)
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(path, size, "bytes")
    assert size < 1 << 20


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN)
