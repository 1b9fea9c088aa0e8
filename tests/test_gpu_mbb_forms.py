"""Every kernel form of the multi-block BiCGStab (one-cell / four-cell per kernel, fused s-t and p-v launches, the updates fused
into the multilevel restriction) gives, bit for bit, what it gave when ``tests/golden/mbb_forms.npz`` was recorded
(``tests/golden/make_golden_mbb_forms.py``, with the one-cell and four-cell kernel families as separate bodies, before they were
written once as ``k_mbb_*<DIMS, W>``).  The recurrence words are exact integer-atomic accumulators (FgDacc), so a solve is reproducible to the bit; a
mismatch means a changed summation or contraction order in one kernel form -- under -ffp-contract=fast that includes which
products the compiler fuses, which follows the shape of the source, not only its arithmetic.

The fp32 library only: the four-cell forms are well-formed in the fp64 build too, but stay switched off there at run time
(mb_bicgstab), so nothing here or elsewhere runs them in doubles."""
import ctypes
import itertools
import os

import numpy as np
import pytest
import torch

from tests import helpers_mb as H

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "mbb_forms.npz")
B = 2
TOL = 1e-6
# FG_MB_BICG_VEC4; 5: p and s four-cell, v, t and x one-cell.  A fused launch is four-cell only when BOTH of its mask bits are set
# (p and v, s and t), so with FUSE 1 / 2 mask 5 runs one-cell kernels throughout (recorded bits equal to mask 0): the mixed mask is
# tested by FUSE = 0, the four-cell fused kernels by mask 31
VEC4 = (0, 31, 5)
FUSE = (0, 1, 2)             # FG_MB_BICG_FUSE
MAX_IT = (1, 2, 7, 5000)     # first iteration, both parities of the ping-pong buffers / accumulator slots, a few iterations, to convergence
FORMS = list(itertools.product(VEC4, FUSE))
# channel40x30: 1200 cells -- four-cell launches of two workgroups (a non-leader one, the last one partly invalid), five one-cell
# workgroups; odd_channel: 77 cells, not divisible by four -- every mask falls back to the one-cell kernels
MESHES = {"channel40x30": lambda: H.split_rotated_channel(nx=40, ny=30), "odd_channel": H.odd_channel}
ML_FUSE = (0, 2)             # FG_MB_ML_FUSE
ML_BICG = (1, 2)             # pressure_use_bicgstab: plain, fp64-refined
ML_DT = [0.05, 0.03]


def solve_form(mesh, A, Coff, rhs):
    """The velocity systems (A [B][N], Coff [B][F][N], rhs [B][d][N]) by fg_mb_debug_bicgstab on a fresh handle, once per entry of
    MAX_IT: x [B][d][N], the accumulator words [B d][12], alpha / omega [B d][2] and the outcome counts of each.  The kernel form
    comes from the environment (read at fg_mb_create)."""
    from fluidgym_amd import _lib as L

    dom = MESHES[mesh]().native(batch=B)
    N, d = dom.n_cells, dom.dims
    lib, hip = L.load(), ctypes.CDLL("libamdhip64.so")
    for which, host in ((L.FG_MB_BUF_A, A), (L.FG_MB_BUF_C_OFF, Coff), (L.FG_MB_BUF_RHS, rhs)):
        ptr, cnt = ctypes.c_void_p(), ctypes.c_int64()
        L.check(lib.fg_mb_get_buffer(dom.handle, which, ctypes.byref(ptr), ctypes.byref(cnt)))
        t = torch.from_numpy(np.ascontiguousarray(host, np.float32)).cuda()
        assert t.numel() == cnt.value
        assert hip.hipMemcpy(ptr, ctypes.c_void_p(t.data_ptr()), ctypes.c_size_t(4 * t.numel()), 3) == 0
    torch.cuda.synchronize()
    res = []
    for k in MAX_IT:
        out = (ctypes.c_int64 * 4)()
        acc = np.zeros((B * d, 12), np.float64)
        sc = np.zeros((B * d, 2), np.float32)
        L.check(lib.fg_mb_debug_bicgstab(dom.handle, TOL, k, 1, out, acc.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                         sc.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), None))
        x = dom.buffer(L.FG_MB_BUF_VELOCITY_RESULT).view(B, d, N).cpu().numpy()
        res.append((x, acc, sc, np.array(out[:], np.int64)))
    dom.close()
    return res


def multilevel_step(bicg, u0, p0):
    """One PISO step on polar_ring with the multilevel-preconditioned pressure BiCGStab (as
    test_multilevel_preconditioned_bicgstab_step_matches_the_oracle): velocity [B][d][N] and pressure [B][N] after it."""
    dom = H.polar_ring().native(batch=B)
    assert dom.set_pressure_multilevel() is not None
    for b in range(B):
        dom.velocity[b] = torch.as_tensor(u0[b], dtype=torch.float32)
        dom.pressure[b] = torch.as_tensor(p0[b], dtype=torch.float32)
    its = dom.piso_step(ML_DT, advection_tol=1e-7, pressure_tol=2e-6, pressure_use_bicgstab=bicg, pressure_project_mean=True)
    assert all(i > 0 for i in its)
    u, p = dom.velocity.cpu().numpy().copy(), dom.pressure.cpu().numpy().copy()
    dom.close()
    return u, p


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("mesh", list(MESHES))
@pytest.mark.parametrize("vec4,fuse", FORMS)
def test_bicgstab_form_reproduces_the_recorded_bits(mesh, vec4, fuse, golden, monkeypatch):
    monkeypatch.setenv("FG_MB_BICG_VEC4", str(vec4))
    monkeypatch.setenv("FG_MB_BICG_FUSE", str(fuse))
    res = solve_form(mesh, golden[mesh + ".A"], golden[mesh + ".Coff"], golden[mesh + ".rhs"])
    f = FORMS.index((vec4, fuse))
    for m, (x, acc, sc, out4) in enumerate(res):
        where = (mesh, vec4, fuse, MAX_IT[m])
        assert np.array_equal(out4, golden[mesh + ".out4"][f, m]), (where, out4)
        assert np.array_equal(_bits(sc), _bits(golden[mesh + ".sc"][f, m])), where
        assert np.array_equal(_bits(acc), _bits(golden[mesh + ".acc"][f, m])), where
        assert np.array_equal(_bits(x), _bits(golden[mesh + ".x_pool"][golden[mesh + ".x_index"][f, m]])), where
    # the solve to convergence is one: converged, finite, and longer than the truncated ones
    assert tuple(res[-1][3][:3]) == (1, 0, 0) and res[-1][3][3] > 7, res[-1][3]


@pytest.mark.parametrize("ml_fuse", ML_FUSE)
@pytest.mark.parametrize("bicg", ML_BICG)
def test_multilevel_bicgstab_step_reproduces_the_recorded_bits(ml_fuse, bicg, golden, monkeypatch):
    """p and s formed inside the restriction (k_ml_restrict_p / _s: the shared heads and the projection means) or by their own
    kernels.  On this small mesh the refined solve (bicg = 2) converges inside its first inner solve -- its recorded bits equal the
    plain solve's -- so the refinement restarts after the first are not reached here; tests/test_gpu_airfoil.py runs those."""
    monkeypatch.setenv("FG_MB_ML_FUSE", str(ml_fuse))
    u, p = multilevel_step(bicg, golden["ml.u0"], golden["ml.p0"])
    i, j = ML_FUSE.index(ml_fuse), ML_BICG.index(bicg)
    assert np.array_equal(_bits(u), _bits(golden["ml.u"][i, j])), (ml_fuse, bicg)
    assert np.array_equal(_bits(p), _bits(golden["ml.p"][i, j])), (ml_fuse, bicg)
