"""``Domain.RestoreEnvs`` / ``fg_env_restore_field`` / ``fg_env_reset_solver_state`` on the GPU, through ``Domain`` directly on small
grids where the tiling can go wrong: rows shorter than the 64-cell tile, just over one tile, a whole number of tiles, and a 3-D grid.
Every comparison is bit for bit: a copy and a sign change do not round."""
import ctypes
import os

import numpy as np
import pytest
import torch

from fluidgym_amd import _lib as L
from fluidgym_amd.simulation import grids
from fluidgym_amd.simulation.domain import Domain
from fluidgym_amd.simulation.state_bank import StateBank, build_selection
from tests.env_restore_ref import restore_ref

pytestmark = pytest.mark.gpu

B = 5
GRIDS = {"2d_6x20": (2, (20, 6)), "2d_3x70": (2, (70, 3)), "2d_16x128": (2, (128, 16)), "3d_5x4x12": (3, (12, 4, 5))}      # (nx, ny[, nz])
DTYPES = [torch.float32, torch.float64]
DT = 0.01


def _need(dtype):
    if dtype == torch.float64 and not os.path.exists(L.LIB_F64_PATH):
        pytest.skip("the fp64 library is not built")


def _make_domain(grid, dtype, fixed=("-y",)):
    """A prepared domain of B envs: walls in y (their face arrays exist), periodic x (and z), one scalar, a velocity source."""
    dims, n = GRIDS[grid] if isinstance(grid, str) else grid
    lengths = [2.0, 1.0, 1.5]
    edges = [np.linspace(0.0, lengths[a], n[a] + 1) for a in range(dims)]
    dom = Domain(dims, 0.05, passiveScalarChannels=1, device="cuda", dtype=dtype, batch=B)
    dom.setScalarViscosity([0.03])
    blk = dom.CreateBlock(vertexCoordinates=grids.vertex_grid(edges))
    for f in fixed:
        blk.CloseBoundary(f)
    dom.PrepareSolve()
    blk.setVelocitySource(torch.zeros(1, dims, *dom.solver.spatial))
    return dom


def _fields(dom):
    """name -> (bound tensor, vector field?) of everything Domain.Clone snapshots."""
    s = dom.solver
    out = {"velocity": (s.velocity, True), "pressure": (s.pressure, False), "scalar": (s.scalar, False),
           "velocity_source": (s.velocity_source, True)}
    out.update({f"bvel{f}": (t, True) for f, t in s.bvel.items()})
    out.update({f"bscal{f}": (t, False) for f, t in s.bscal.items()})
    return out


def _randomise(dom, seed, scale=0.3):
    g = torch.Generator(device="cuda").manual_seed(seed)
    for name, (t, _) in _fields(dom).items():
        t.copy_(scale * torch.randn(t.shape, device=t.device, dtype=t.dtype, generator=g))
    for f, t in dom.solver.bvel.items():
        t[:, f >> 1] = 0.0          # no flux through the walls
    dom.solver.reset_solver_state()


def _random_bank(dom, S, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    s = dom.solver
    r = lambda t: 0.3 * torch.randn((1,) + tuple(t.shape[1:]), device=t.device, dtype=t.dtype, generator=g)
    snaps = []
    for _ in range(S):
        snap = {"velocity": r(s.velocity), "pressure": r(s.pressure), "scalar": r(s.scalar), "velocity_source": r(s.velocity_source),
                "bvel": {f: r(t) for f, t in s.bvel.items()}, "bscal": {f: r(t) for f, t in s.bscal.items()}}
        for f, t in snap["bvel"].items():
            t[:, f >> 1] = 0.0
        snaps.append(snap)
    return StateBank(snaps)


def _bank_arrays(bank):
    out = {k: t.cpu().numpy() for k, t in bank.fields.items()}
    out.update({f"bvel{f}": t.cpu().numpy() for f, t in bank.bvel.items()})
    out.update({f"bscal{f}": t.cpu().numpy() for f, t in bank.bscal.items()})
    return out


def _host(dom):
    return {k: t.detach().cpu().numpy().copy() for k, (t, _) in _fields(dom).items()}


def _solver_buffers(dom):
    s = dom.solver
    return (s.buffer(L.FG_BUF_P_RESULT, (s.B, 1) + tuple(s.spatial)).cpu().numpy(),
            s.buffer(L.FG_BUF_VEL_RESULT, (s.B, s.dims) + tuple(s.spatial)).cpu().numpy())


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _step(dom):
    ok, _ = dom.solver.piso_step(DT, advection_tol=1e-6, pressure_tol=1e-6)
    assert ok


def _mixed_plan(dims, nx, nz, S):
    """Envs {1, 3}: one mirrored in x and rolled to the last cell, one (in 3-D) mirrored in z, rolled in both."""
    plan = dict(envs=[1, 3], src=[S - 1, 0], flip_x=[1, 0], shift_x=[nx - 1, nx // 3 + 1])
    if dims == 3:
        plan.update(flip_z=[0, 1], shift_z=[nz - 1, 2])
    return plan


def _expected(before, bank, dom, plan):
    kw = {k: plan.get(k) for k in ("flip_x", "flip_z", "shift_x", "shift_z")}
    arrays = _bank_arrays(bank)
    return {k: restore_ref(before[k], arrays[k], dom.dims, plan["envs"], plan["src"], signed=signed, **kw)
            for k, (_, signed) in _fields(dom).items()}


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp64"])
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("grid", list(GRIDS))
def test_chosen_envs_equal_the_reference_and_the_others_are_untouched(grid, S, dtype):
    _need(dtype)
    dom = _make_domain(grid, dtype)
    s = dom.solver
    _randomise(dom, seed=1)
    _step(dom)                                   # pressureResult / velocityResult of every env now hold a solve's values
    bank = _random_bank(dom, S, seed=2)
    before, (p_before, u_before) = _host(dom), _solver_buffers(dom)
    assert np.abs(p_before).max() > 0
    plan = _mixed_plan(dom.dims, s.nx, s.nz, S)
    dom.RestoreEnvs(bank, **plan)
    torch.cuda.synchronize()
    after, (p_after, u_after) = _host(dom), _solver_buffers(dom)
    want = _expected(before, bank, dom, plan)
    for k in want:
        assert _same(after[k], want[k]), k       # the chosen envs: the reference; the others: what they were (restore_ref keeps them)
        assert not _same(after[k][plan["envs"]], before[k][plan["envs"]]), k
    others = [e for e in range(B) if e not in plan["envs"]]
    assert _same(p_after[others], p_before[others]) and _same(u_after[others], u_before[others])
    assert not p_after[plan["envs"]].any()
    assert _same(u_after[plan["envs"]], after["velocity"][plan["envs"]])
    s.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp64"])
@pytest.mark.parametrize("grid", ["2d_3x70", "3d_5x4x12"])
def test_all_envs_with_identity_transforms_equal_restore(grid, dtype):
    _need(dtype)
    dom = _make_domain(grid, dtype)
    s = dom.solver
    _randomise(dom, seed=3)
    snap = dom.Clone()
    bank = StateBank([snap])                     # every env an entry of its own: S = B
    assert bank.size == B
    results = []
    for restore in (lambda: dom.RestoreEnvs(bank, list(range(B)), list(range(B))),
                    lambda: (dom.Restore(snap), s.reset_solver_state())):
        _randomise(dom, seed=4)
        _step(dom)
        restore()
        torch.cuda.synchronize()
        results.append((_host(dom), _solver_buffers(dom)))
    (f_a, (p_a, u_a)), (f_b, (p_b, u_b)) = results
    for k in f_a:
        assert _same(f_a[k], f_b[k]), k
        assert _same(f_a[k], snap[k].cpu().numpy() if k in snap else snap[k[:-1]][int(k[-1])].cpu().numpy()), k
    assert _same(p_a, p_b) and _same(u_a, u_b) and not p_a.any()
    s.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp64"])
@pytest.mark.parametrize("grid", list(GRIDS))
def test_replay_restore_envs_then_step_equals_restore_of_the_composed_state(grid, dtype):
    """Batch A: step, RestoreEnvs, two steps.  Batch B: the same step, then the composed fields through Domain.Restore with A's solver
    hints and the same per-env solver-state reset, two steps.  Bit for bit: every reduction of the step is order-independent."""
    _need(dtype)
    doms = [_make_domain(grid, dtype) for _ in range(2)]
    for dom in doms:
        _randomise(dom, seed=5, scale=0.2)
        _step(dom)
    A, Bd = doms
    bank = _random_bank(A, 3, seed=6)
    for t in list(bank.fields.values()) + list(bank.bvel.values()):
        t.mul_(0.5)
    plan = _mixed_plan(A.dims, A.solver.nx, A.solver.nz, 3)
    before = _host(A)
    for k, v in _host(Bd).items():
        assert _same(v, before[k]), k            # the two batches agree before anything is restored
    sel = A.RestoreEnvs(bank, **plan)
    want = _expected(before, bank, A, plan)
    to_dev = lambda a: torch.from_numpy(a).to("cuda")
    snap = {k: to_dev(want[k]) for k in ("velocity", "pressure", "scalar", "velocity_source")}
    snap["bvel"] = {f: to_dev(want[f"bvel{f}"]) for f in Bd.solver.bvel}
    snap["bscal"] = {f: to_dev(want[f"bscal{f}"]) for f in Bd.solver.bscal}
    hints = Bd.solver.solver_hints()
    assert hints == A.solver.solver_hints()      # RestoreEnvs leaves the handle's hints alone
    snap["solver_hints"] = hints
    Bd.Restore(snap)
    Bd.solver.env_reset_solver_state(sel)
    for _ in range(2):
        _step(A)
        _step(Bd)
    torch.cuda.synchronize()
    a, b = _host(A), _host(Bd)
    for k in a:
        assert np.isfinite(a[k]).all(), k
        assert _same(a[k], b[k]), k
    pa, pb = _solver_buffers(A), _solver_buffers(Bd)
    assert _same(pa[0], pb[0]) and _same(pa[1], pb[1])
    for dom in doms:
        dom.solver.close()


def _records(*rows):
    sel = (L.FgEnvSel * len(rows))()
    for i, r in enumerate(rows):
        sel[i] = L.FgEnvSel(*r)
    return sel


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp64"])
def test_every_refusal_returns_its_error_and_changes_nothing(dtype):
    _need(dtype)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for grid, fixed, bad in [
        ("2d_6x20", ("-y",), [
            [(5, 0, 0, 0, 0, 0)], [(-1, 0, 0, 0, 0, 0)],                    # env out of range
            [(1, 3, 0, 0, 0, 0)], [(1, -1, 0, 0, 0, 0)],                    # src out of range (S = 3)
            [(1, 0, 0, 0, 0, 0), (1, 1, 0, 0, 0, 0)],                       # an env twice
            [(e % B, 0, 0, 0, 0, 0) for e in range(B + 1)],                 # n_sel > B
            [(1, 0, 0, 0, 20, 0)], [(1, 0, 0, 0, -1, 0)],                   # shift outside [0, nx)
            [(1, 0, 2, 0, 0, 0)],                                           # a flip is 0 or 1
            [(1, 0, 0, 1, 0, 0)], [(1, 0, 0, 0, 0, 1)],                     # z on a 2-D grid
        ]),
        ((2, (20, 6)), ("-x", "-y"), [[(1, 0, 1, 0, 0, 0)], [(1, 0, 0, 0, 3, 0)]]),           # x has FIXED faces
        ((3, (12, 4, 5)), ("-y", "-z"), [[(1, 0, 0, 1, 0, 0)], [(1, 0, 0, 0, 0, 2)], [(1, 0, 0, 0, 0, 5)]]),      # z has FIXED faces
    ]:
        dom = _make_domain(grid, dtype, fixed)
        s = dom.solver
        _randomise(dom, seed=7)
        bank = _random_bank(dom, 3, seed=8)
        before, buffers = _host(dom), _solver_buffers(dom)
        call = lambda sel, which=L.FG_VELOCITY, signed=1: s.lib.fg_env_restore_field(
            s.handle, which, ctypes.c_void_p(bank.fields["velocity"].data_ptr()), 3, sel, len(sel), signed, stream)
        for rows in bad:
            assert call(_records(*rows)) == L.FG_ERR_INVALID_ARG, rows
            assert s.lib.fg_last_error()
        good = _records((1, 0, 0, 0, 0, 0))
        assert call(good, which=7) == L.FG_ERR_INVALID_ARG                 # no such field
        assert call(good, which=L.FG_PRESSURE, signed=1) == L.FG_ERR_INVALID_ARG      # a sign rule on a scalar field
        assert s.lib.fg_env_restore_field(s.handle, L.FG_VELOCITY, None, 3, good, 1, 1, stream) == L.FG_ERR_INVALID_ARG
        assert s.lib.fg_env_restore_field(s.handle, L.FG_VELOCITY, ctypes.c_void_p(bank.fields["velocity"].data_ptr()), 0, good, 1, 1,
                                          stream) == L.FG_ERR_INVALID_ARG
        for rows in ([(5, 0, 0, 0, 0, 0)], [(1, 0, 0, 0, 0, 0), (1, 0, 0, 0, 0, 0)], [(e % B, 0, 0, 0, 0, 0) for e in range(B + 1)]):
            assert s.lib.fg_env_reset_solver_state(s.handle, _records(*rows), len(rows), stream) == L.FG_ERR_INVALID_ARG
        # the Python door refuses the same before it reaches the library
        with pytest.raises(ValueError):
            dom.RestoreEnvs(bank, [1, 1], [0, 0])
        with pytest.raises(ValueError):
            dom.RestoreEnvs(bank, [1], [0], shift_x=[s.nx])
        with pytest.raises(ValueError):
            dom.RestoreEnvs(bank, [1], [0], **({"flip_x": 1} if "-x" in fixed else {"flip_z": 1} if "-z" in fixed or s.dims == 2 else {"src": 9}))
        torch.cuda.synchronize()
        after, buffers_after = _host(dom), _solver_buffers(dom)
        for k in before:
            assert _same(after[k], before[k]), k
        assert _same(buffers[0], buffers_after[0]) and _same(buffers[1], buffers_after[1])
        s.close()
    assert s.lib.fg_mb_env_restore_field(None, 0, None, 1, None, 1, 0, None) == L.FG_ERR_UNSUPPORTED
