"""Every launched form of the chunked multi-block pressure CG (``csrc/fg_mb_krylov.hip::mb_cg``: one or four cells per thread, the
three residual projections, 2-D and 3-D, the multilevel-preconditioned recurrence, in the fp32 and the fp64 library) gives, bit for
bit, what it gave when ``tests/golden/mbc_forms.npz`` was recorded (``tests/golden/make_golden_mbc_forms.py``, with the recurrence
written three times -- k_mbc_ap / k_mbc_ap4 / k_mbc_ap_pre and their update kernels -- and the iteration index in a device counter,
before the kernels were written once as ``k_mbc_ap<DIMS, W, ...>`` / ``k_mbc_update<W, PRE>``).  Every sum of the recurrence is a
fixed-order workgroup tree into exact integer-atomic accumulators (FgDacc), so a solve is reproducible to the bit; a mismatch means a
changed summation or contraction order -- under -ffp-contract=fast that includes which products the compiler fuses, which follows
the shape of the source, not only its arithmetic.

The on-chip and the cluster CG are switched off (FG_MB_ONCHIP=0, FG_MB_CLUSTER=0), so ``Domain.debug_pressure_cg`` lands in the chunked
solver.  Compared per case and iteration cap: the five Krylov work arrays (FG_MB_BUF_KRYLOV0..4 = residual, the two direction
buffers, A p, the kept iterate -- as SHA-256 digests of their bytes, the fixture has no room for the arrays), and the iterations /
converged / residual words of every env.  That pins the trajectory, not that x solves the system: the solver's own pressure array x
(FG_MB_BUF_PRESSURE_X) is read behind each of these solves by tests/test_gpu_mb_cg_solutions.py and held to the fp64 residual it
leaves in the system, at every cap -- the kept iterate of the caps 20 and 40, the iterate behind the restart of cap 120, the
converged one with its updates behind the last kept iterate and the last restart.  Here x is held through what is computed from it:
the kept iterate is a copy of x (of the iteration that last halved the residual; what an unconverged solve hands back), and every
restart of the recurrence (iteration 100, 200, ...) recomputes r = b - A x from x, so all work arrays of the caps 120 and 5000
depend on every bit of x up to their last restart.  W = 1 on a 3-D mesh (no mesh of this fixture: every 3-D one has a cell count
divisible by four) runs there as well, on ``helpers_mb.odd_channel_3d``, against its fp64 residual and the oracle.
Not covered, here or there: the breakdown recovery (k_mbs_recover: no system of the fixture breaks down), the cluster CG's give-up
path (a granule that hands the solve back to the one-workgroup kernels), and z of the preconditioned recurrence (no buffer id
exposes it; r, p and A p depend on every bit of it)."""
import ctypes
import hashlib
import os

import numpy as np
import pytest
import torch

from tests import helpers_mb as H

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "mbc_forms.npz")
B = 2
# mb_cg rounds the cap up to whole chunks of 20: 20 and 40 end unconverged (k_mbs_restore_best, the keep-best copy), 120 crosses the
# restart of the recurrence at iteration 100, 5000 runs to convergence
CAPS = (20, 40, 120, 5000)
N_WORK = 5
# channel40x30: 1200 cells -- W = 4 in the fp32 library: two workgroups (a non-leader one, the last one partly invalid), +-x
# neighbours across lanes and across the block cut; five one-cell workgroups in the fp64 library.  channel41x30: 1230 cells, not
# divisible by four -- W = 1 over several workgroups.  odd_channel: 77 cells, W = 1 in one workgroup.  skewed_pair_3d: DIMS = 3
MESHES = {
    "channel40x30": lambda: H.split_rotated_channel(nx=40, ny=30),
    "channel41x30": lambda: H.split_rotated_channel(nx=41, ny=30),
    "odd_channel": H.odd_channel,
    "skewed_pair_3d": H.skewed_pair_3d,
    "polar_ring": H.polar_ring,
}
# (library, mesh, multilevel-preconditioned recurrence, residual projections: 0 none, 1 the constant, 2 a general unit vector)
GROUPS = [
    ("f32", "channel40x30", False, (0, 1, 2)),
    ("f32", "channel41x30", False, (0, 1, 2)),
    ("f32", "odd_channel", False, (0, 1, 2)),
    ("f32", "skewed_pair_3d", False, (1,)),
    ("f32", "polar_ring", True, (0, 1)),
    # the instances float64 envs run in production
    ("f64", "channel40x30", False, (0, 1, 2)),
    ("f64", "polar_ring", True, (0, 1)),
]
CASES = [(lib, mesh, pre, pm) for lib, mesh, pre, pms in GROUPS for pm in pms]
SWITCHES = {"FG_MB_ONCHIP": "0", "FG_MB_CLUSTER": "0", "FG_MB_PCG_KERNEL": "1"}   # read at fg_mb_create


def case_key(lib, mesh, pre, pm):
    return f"{lib}.{mesh}.pm{pm}"


def open_case(lib, mesh, pre, pm, diag, off, rhs, yp):
    """A fresh handle with the pressure systems (diag [B][N], off [B][F][N], rhs [B][N]) uploaded into its pressure buffers, the
    multilevel tables and the residual projection installed as the case asks.  SWITCHES must be in the environment."""
    from fluidgym_amd import _lib as L

    dtype = torch.float64 if lib == "f64" else torch.float32
    dom = MESHES[mesh]().native(batch=B, dtype=dtype)
    if pre:   # (before the matrix goes in: the tables are built from the unit pressure matrix, through the same buffers)
        assert dom.set_pressure_multilevel(fp64=(lib == "f64")) is not None
    if pm == 2:
        y = np.ascontiguousarray(yp, dom._np)
        L.check(dom.lib.fg_mb_set_residual_projection(dom.handle, y.ctypes.data_as(ctypes.POINTER(dom._cf))))
    hip = ctypes.CDLL("libamdhip64.so")
    for which, host in ((L.FG_MB_BUF_P_DIAG, diag), (L.FG_MB_BUF_P_OFF, off), (L.FG_MB_BUF_DIV, rhs)):
        ptr, cnt = ctypes.c_void_p(), ctypes.c_int64()
        L.check(dom.lib.fg_mb_get_buffer(dom.handle, which, ctypes.byref(ptr), ctypes.byref(cnt)))
        t = torch.from_numpy(np.ascontiguousarray(host, dom._np)).cuda()
        assert t.numel() == cnt.value
        assert hip.hipMemcpy(ptr, ctypes.c_void_p(t.data_ptr()), ctypes.c_size_t(t.element_size() * t.numel()), 3) == 0
    torch.cuda.synchronize()
    return dom


def solve_case(lib, mesh, pre, pm, diag, off, rhs, yp, tol):
    """The pressure systems by ``debug_pressure_cg`` on a fresh handle (``open_case``), once per entry of CAPS: the digests of the work
    arrays and the outcome words of each."""
    from fluidgym_amd import _lib as L

    dom = open_case(lib, mesh, pre, pm, diag, off, rhs, yp)
    N = dom.n_cells
    res = []
    for cap in CAPS:
        info = dom.debug_pressure_cg(tol, cap, project_mean=(pm != 0))
        work = np.stack([np.frombuffer(hashlib.sha256(dom.buffer(L.FG_MB_BUF_KRYLOV0 + k)[:B * N].cpu().numpy().tobytes()).digest(), np.uint8)
                         for k in range(N_WORK)])
        res.append({"work": work, "iterations": np.array(info["iterations"], np.int32),
                    "converged": np.array(info["converged"], np.uint8), "residual": np.array(info["residual"], np.float64)})
    dom.close()
    return res


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("lib,mesh,pre,pm", CASES)
def test_chunked_cg_reproduces_the_recorded_bits(lib, mesh, pre, pm, golden, monkeypatch):
    for k, v in SWITCHES.items():
        monkeypatch.setenv(k, v)
    key = case_key(lib, mesh, pre, pm)
    g_it, g_conv = golden[key + ".iterations"], golden[key + ".converged"]
    # the fixture itself reached what it is there for: the long solve of the 1200-cell mesh converged, and only behind the restart of
    # the recurrence at iteration 100; the preconditioned solve ran into its second chunk
    if mesh == "channel40x30" and pm == 1:
        assert g_conv[-1].all() and (g_it[-1] > 100).all(), (key, g_it[-1], g_conv[-1])
    if pre:
        assert (g_it[-1] > 20).all(), (key, g_it[-1])
    res = solve_case(lib, mesh, pre, pm, golden[mesh + ".diag"], golden[mesh + ".off"], golden[mesh + ".rhs"], golden[mesh + ".yp"],
                     float(golden["tol." + lib]))
    for m, r in enumerate(res):
        where = (key, CAPS[m])
        print(where, "iterations", r["iterations"].tolist(), "converged", r["converged"].tolist(), "residual", r["residual"].tolist())
        assert np.array_equal(r["iterations"], g_it[m]), (where, r["iterations"], g_it[m])
        assert np.array_equal(r["converged"], g_conv[m]), (where, r["converged"], g_conv[m])
        assert np.array_equal(_bits(r["residual"]), _bits(golden[key + ".residual"][m])), (where, r["residual"], golden[key + ".residual"][m])
        same = [bool(np.array_equal(r["work"][k], golden[key + ".work"][m][k])) for k in range(N_WORK)]
        assert all(same), (where, "work arrays r, pA, pB, Ap, best_x equal:", same)
