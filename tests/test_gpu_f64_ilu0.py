"""ILU(0) in the fp64 build (libfluidgym_hip_f64.so, csrc/fg_ilu0.hip compiled with fg_real = double): the preconditioner of the
reference's advection-diffusion rungs for double fields -- ``preconditionBiCG`` / ``BiCG_precondition_fallback``, cusparseDcsrilu02 +
two SpSV per application (bicgstab_solver_kernel.cu:191-226; PISOtorch_diff.py:449-476).  The y-line and Helmholtz preconditioners
are fp32 kernel families; on this build ``Simulation`` maps the two flags onto modes 4 / 5 (tests/test_f64_rung_mapping.py).

Held against a generic IKJ ILU(0) in NumPy of the matrix the GPU assembled (to 1e-12 now that rounding no longer hides an error of
the kernel), against direct fp64 solves, against the reference's recorded ladder sequences and against the fp64 oracle's step."""
import numpy as np
import pytest
import torch

from fluidgym_amd import _lib as L
from oracle import piso_oracle as O
from tests.helpers import make_case, rel_err
from tests.test_control_golden import GOLDEN, ladder_attempts

pytestmark = pytest.mark.gpu

F64 = torch.float64


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _wall_refined(case, ratio):
    """Replace the y widths by a two-sided geometric wall refinement (largest / smallest width = ratio)."""
    ny = len(case.widths[1])
    half = ny // 2
    g = ratio ** (1.0 / max(half - 1, 1))
    w = np.concatenate([g ** np.arange(half), g ** np.arange(ny - half)[::-1]])
    w = (w / w.sum()).astype(np.float32)
    case.widths[1] = w
    case.edges[1] = np.concatenate([[0.0], np.cumsum(w.astype(np.float64))])
    return case


def _dense_from_stencil(A, off, shape, periodic):
    """Dense matrix of one env from the GPU's buffers: A [N], off [2d, N]; cells in natural order (x fastest)."""
    dims = len(shape)                     # shape = (ny, nx) or (nz, ny, nx)
    ext = list(shape[::-1])               # [nx, ny(, nz)]
    N = int(np.prod(ext))
    M = np.zeros((N, N))
    pattern = np.zeros((N, N), bool)
    idx = np.arange(N)
    pos = [idx % ext[0], (idx // ext[0]) % ext[1]] + ([idx // (ext[0] * ext[1])] if dims == 3 else [])
    M[idx, idx] = A
    pattern[idx, idx] = True
    stride = [1, ext[0], ext[0] * ext[1]]
    for f in range(2 * dims):
        ax, up = f >> 1, f & 1
        p = pos[ax] + (1 if up else -1)
        inside = (p >= 0) & (p < ext[ax])
        wrap = ~inside & periodic[ax]
        nb = np.where(inside, idx + (1 if up else -1) * stride[ax], np.where(up, idx - (ext[ax] - 1) * stride[ax], idx + (ext[ax] - 1) * stride[ax]))
        ok = inside | wrap
        M[idx[ok], nb[ok]] += off[f][ok]
        pattern[idx[ok], nb[ok]] = True
    return M, pattern


def _ilu0_generic(M, pattern):
    """IKJ incomplete LU without fill on `pattern` (Saad, Iterative Methods, alg. 10.4); returns unit-lower L and upper U."""
    n = M.shape[0]
    LU = M.copy()
    for i in range(1, n):
        for k in np.nonzero(pattern[i, :i])[0]:
            LU[i, k] /= LU[k, k]
            js = np.nonzero(pattern[i, k + 1:])[0] + k + 1
            LU[i, js] -= LU[i, k] * np.where(pattern[k, js], LU[k, js], 0.0)
    return np.tril(LU, -1) + np.eye(n), np.triu(LU)


def _direct(case, b, dt, g):
    dom = case.oracle_domain(b, g)
    C, _, _ = O.build_advection_matrix(dom, dt)
    rhs = O.advection_rhs_velocity(dom, dt)
    return [O.solve_direct(C, rhs[comp].ravel()).reshape(case.shape) for comp in range(case.dims)]


@pytest.mark.parametrize("dims,n,fixed_axes", [(2, (12, 10), (1,)), (2, (9, 8), (0, 1)), (2, (8, 12), ()), (3, (6, 5, 4), (1,)),
                                               (3, (5, 4, 6), (0, 1, 2))])
def test_fp64_ilu0_application_is_the_generic_incomplete_factorisation(dims, n, fixed_axes):
    case = make_case(dims=dims, n=n, fixed_axes=fixed_axes, B=2, seed=5, nu=0.05, vel_scale=0.5)
    ns = case.native(dtype=F64)
    ns.setup_advection(0.05)
    A = _np(ns.buffer(L.FG_BUF_A, (case.B, -1)))
    off = _np(ns.buffer(L.FG_BUF_C_OFF, (case.B, 2 * dims, -1)))
    g = torch.Generator(device="cpu").manual_seed(3)
    r = torch.randn((case.B, dims) + case.shape, generator=g, dtype=F64)
    z = ns.apply_advection_preconditioner(4, r)
    assert z.dtype == F64
    z = _np(z).reshape(case.B, dims, -1)
    ns.close()
    periodic = [a not in fixed_axes for a in range(dims)]
    worst = 0.0
    for b in range(case.B):
        M, pattern = _dense_from_stencil(A[b], off[b], case.shape, periodic)
        Lm, U = _ilu0_generic(M, pattern)
        offd = ~np.eye(M.shape[0], dtype=bool)
        assert np.abs((np.triu(U, 1) - np.triu(M, 1)))[offd].max() <= 1e-12 * np.abs(M).max()
        for comp in range(dims):
            z_ref = np.linalg.solve(U, np.linalg.solve(Lm, r[b, comp].numpy().ravel()))
            worst = max(worst, rel_err(z[b, comp], z_ref))
            assert rel_err(z[b, comp], z_ref) <= 1e-12, (b, comp, rel_err(z[b, comp], z_ref))
    print(f"F64_ILU0 apply dims={dims} n={n} fixed={fixed_axes}: rel err {worst:.1e}")


def test_fp64_ilu0_preconditioned_solve_matches_the_direct_solve_in_fewer_iterations():
    case = _wall_refined(make_case(dims=2, n=(64, 48), fixed_axes=(1,), B=2, seed=4, nu=0.05, vel_scale=0.3), ratio=10.0)
    dt, tol = 0.05, 1e-12
    out = {}
    for mode in (0, 4):
        ns = case.native(dtype=F64)
        ns.set_advection_start(False)
        ns.set_advection_preconditioner(mode)
        ns.setup_advection(dt)
        info = ns.solve_advection(tol=tol)
        assert all(i.converged and i.is_finite for i in info), (mode, [i.final_residual for i in info])
        out[mode] = (_np(ns.buffer(L.FG_BUF_VEL_RESULT, (case.B, case.dims) + case.shape)), max(i.used_iterations for i in info) + 1)
        ns.close()
    g = case.grid()
    for b in range(case.B):
        for comp, x_ref in enumerate(_direct(case, b, dt, g)):
            for mode in (0, 4):
                assert rel_err(out[mode][0][b, comp], x_ref) < 1e-10, (mode, b, comp, rel_err(out[mode][0][b, comp], x_ref))
    print(f"F64_ILU0 iterations to {tol:g}: plain {out[0][1]}, ILU(0) {out[4][1]}")
    assert out[4][1] < out[0][1], (out[0][1], out[4][1])


def test_fp64_ilu0_fallback_rung_rescues_a_system_the_plain_recurrence_cannot_solve_within_its_cap():
    """Mode 5 (BiCG_precondition_fallback) on the 60 : 1 wall-refined system: the plain fp64 recurrence does not reach the tolerance
    within the cap (it needs 550-610 iterations to 1e-12), the rung repeats the solve from zero with ILU(0) (18-20 iterations) and
    converges, once, on the direct solve."""
    case = _wall_refined(make_case(dims=2, n=(64, 48), fixed_axes=(1,), B=2, seed=4, nu=0.05, vel_scale=0.3), ratio=60.0)
    dt, tol, cap = 0.05, 1e-12, 60
    ns = case.native(dtype=F64)
    ns.set_advection_start(False)
    ns.set_advection_preconditioner(0)
    ns.setup_advection(dt)
    assert not all(i.converged for i in ns.solve_advection(tol=tol, max_iterations=cap))
    ns.set_advection_preconditioner(5)
    ns.ladder(force_mask=0)
    before = ns.ladder()
    info = ns.solve_advection(tol=tol, max_iterations=cap)
    assert all(i.converged and i.is_finite for i in info), [i.final_residual for i in info]
    after = ns.ladder()
    assert ns.advection_retries() == 1
    assert after["advection_preconditioned"] - before["advection_preconditioned"] == 1 and after["advection_fp64"] == 0, after
    x = _np(ns.buffer(L.FG_BUF_VEL_RESULT, (case.B, case.dims) + case.shape))
    ns.close()
    print(f"F64_ILU0 fallback: rung iterations {max(i.used_iterations for i in info) + 1} (cap {cap})")
    g = case.grid()
    for b in range(case.B):
        for comp, x_ref in enumerate(_direct(case, b, dt, g)):
            assert rel_err(x[b, comp], x_ref) < 1e-10, (b, comp)


def test_fp64_ilu0_refuses_axes_shorter_than_four_cells():
    case = make_case(dims=2, n=(3, 8), fixed_axes=(1,), B=1, seed=1)
    ns = case.native(dtype=F64)
    with pytest.raises(L.NativeLibraryError, match="four cells"):
        ns.set_advection_preconditioner(4)
    with pytest.raises(L.NativeLibraryError, match="four cells"):
        ns.set_advection_preconditioner(5)
    ns.close()


# ---- the reference's ladder on the fp64 build --------------------------------------------------------------------------------
LADDER_CASES = {"2d": dict(dims=2, n=(32, 24), fixed_axes=(1,), B=2, seed=41), "3d": dict(dims=3, n=(16, 12, 8), fixed_axes=(1,), B=2, seed=42)}
LADDER_KW = dict(advection_tol=1e-12, pressure_tol=1e-12)
FORCE = {"advection": 1, "pressure": 2}


def _ladder_step(case, double_fallback, precond_mode, force, dt=0.05):
    ns = case.native(dtype=F64)
    ns.set_double_fallback(double_fallback)
    ns.set_advection_preconditioner(precond_mode)
    ns.ladder(force_mask=force)
    ok, stats = ns.piso_step(dt, **LADDER_KW)
    used = ns.ladder(force_mask=0)
    u, p = _np(ns.velocity), _np(ns.pressure)
    ns.close()
    return ok, used, u, p


@pytest.mark.parametrize("which", list(LADDER_CASES))
def test_fp64_ladder_runs_the_preconditioned_rung_exactly_when_the_reference_does(which):
    """The 72 recorded sequences of tests/golden/reference_control.json replayed on the fp64 build with the rung as mode 5.  The
    reference skips its fp64 re-solve for double fields (``double_fallback and rhs.dtype == torch.float32``, PISOtorch_diff.py:418),
    so what it runs for fp64 fields is the recorded sequence of the same configuration with double_fallback off: the fp64 re-solve
    dropped, and the next scripted outcome goes to the preconditioned attempt.  The fp64 build accepts solver_double_fallback and has
    nothing to fall back to; every rung lands on the plain fp64 step."""
    case = make_case(vel_scale=0.4, nu=0.03, with_source=True, **LADDER_CASES[which])
    ok, used, u_plain, p_plain = _ladder_step(case, False, 0, 0)
    assert ok and used == {"advection_fp64": 0, "advection_preconditioned": 0, "pressure_fp64": 0}
    seen = set()
    n_rung = n_checked = 0
    for c in GOLDEN["ladder"]:
        use_bicg, rbr, dfb, pfb = c["use_bicg"], c["return_best_result"], c["double_fallback"], c["precondition_fallback"]
        kind = "advection" if (use_bicg and not rbr) else ("pressure" if (not use_bicg and rbr) else None)
        if kind is None:
            continue        # (BiCGStab with returnBestResult / CG without: combinations the step never issues)
        ref = ladder_attempts(use_bicg, rbr, False, pfb, c["scripted_outcomes"])      # what the reference runs for fp64 fields
        assert all(a["dtype"] == "float32" for a in ref["attempts"])
        rungs = tuple("preconditioned" if a["preconditioned"] else "plain" for a in ref["attempts"][1:])
        first = c["scripted_outcomes"][0]
        failed_first = (first != "converged") if kind == "advection" else (first == "non_finite")
        force = FORCE[kind] if failed_first else 0
        key = (kind, dfb, pfb, force)
        if key in seen:
            continue
        seen.add(key)
        ok, used, u, p = _ladder_step(case, dfb, 5 if pfb else 0, force)
        expect = int(rungs == ("preconditioned",))
        assert int(used["advection_preconditioned"] > 0) == expect, (c, ref["attempts"], used)
        assert used["advection_fp64"] == 0 and used["pressure_fp64"] == 0, (c, used)
        assert np.isfinite(u).all() and np.isfinite(p).all()
        for b in range(case.B):
            assert rel_err(u[b], u_plain[b]) < 1e-9, (c, b, rel_err(u[b], u_plain[b]))
            assert rel_err(p[b, 0] - p[b, 0].mean(), p_plain[b, 0] - p_plain[b, 0].mean()) < 1e-8, (c, b)
        n_rung += expect
        n_checked += 1
    assert n_checked >= 8 and n_rung >= 2, (n_checked, n_rung)


# ---- Simulation(...) with the reference's flags on fp64 single-block domains ----------------------------------------------------
SIM_CASES = [dict(dims=2, n=(32, 24), fixed_axes=(1,), B=2, seed=5, with_source=True),
             dict(dims=3, n=(12, 10, 8), fixed_axes=(1,), B=2, seed=7)]
_FACES = ("-x", "+x", "-y", "+y", "-z", "+z")


def _sim_domain(case):
    from fluidgym_amd.simulation import Domain, grids

    dom = Domain(case.dims, torch.tensor([case.nu], dtype=F64), dtype=F64, batch=case.B)   # (nu in double, as the oracle has it)
    blk = dom.CreateBlock(grids.vertex_grid(case.edges, dtype=F64))
    for f in case.fixed_faces:
        blk.CloseBoundary(_FACES[f], velocity=torch.from_numpy(case.bvel[f]))
    blk.setVelocity(torch.from_numpy(case.velocity))
    if case.source is not None:
        blk.setVelocitySource(torch.from_numpy(case.source))
    dom.PrepareSolve()
    assert dom.solver.f64
    return dom


@pytest.mark.parametrize("kw", SIM_CASES)
@pytest.mark.parametrize("flags", [dict(preconditionBiCG=True), dict(BiCG_precondition_fallback=True)])
def test_fp64_simulation_with_the_reference_flags_constructs_and_steps(kw, flags):
    from fluidgym_amd.simulation import Simulation

    case = make_case(vel_scale=0.4, nu=0.03, **kw)
    dom = _sim_domain(case)
    dt = 0.03
    sim = Simulation(dom, dt, substeps=1, advection_tol=1e-13, pressure_tol=1e-13, **flags)
    assert sim.advection_preconditioner == (4 if flags.get("preconditionBiCG") else 5)
    solver = dom.solver
    assert sim.single_step()
    if flags.get("preconditionBiCG"):
        # one step from the case's state: the fp64 oracle's, at the gate of tests/test_gpu_f64.py (velocity 1e-10, pressure 1e-9)
        g = case.grid()
        for b in range(case.B):
            ref = case.oracle_domain(b, g)
            O.piso_split_step(ref, dt)
            p = _np(solver.pressure[b, 0])
            eu, ep = rel_err(_np(solver.velocity[b]), ref.velocity), rel_err(p - p.mean(), ref.pressure - ref.pressure.mean())
            print(f"F64_ILU0 Simulation(preconditionBiCG) dims={case.dims} env {b}: velocity {eu:.1e} pressure {ep:.1e} {sim.last_stats}")
            assert eu < 1e-10 and ep < 1e-9, (b, eu, ep)
    for _ in range(3):
        assert sim.single_step()
    assert torch.isfinite(solver.velocity).all() and torch.isfinite(solver.pressure).all()
    solver.close()
