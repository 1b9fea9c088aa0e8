"""Kernel parity with a non-zero normal velocity on every fixed face (``tests/helpers.py::with_normal_flux``).

``make_case`` zeroes the wall-normal component of every boundary velocity, so in the other kernel-level tests every term a kernel
multiplies by the boundary normal flux ``U_b`` is multiplied by zero (the +-x faces of two 2-D cases excepted): the ``u_b U_b`` /
``t_b U_b`` terms of ``k_adv_build`` on y and z faces, the boundary fluxes of ``k_div`` and of the fused pressure row kernel, the
slab scans of the CFL maximum and the signs and area weights of the flux balance.  Here they all carry through-flow -- what the
TCF envs' wall-normal blowing and suction is -- and meet the oracle at the gates of the tests they mirror (``test_gpu_parity.py``,
``test_gpu_sgs.py``, ``test_gpu_f64.py``, ``test_gpu_fused_cg.py``).  The inputs' own conditions (balanced fluxes, unchanged
matrix, right-hand sides that move by O(1)) are checked on the host in ``tests/test_normal_flux_inputs.py``."""
import functools

import numpy as np
import pytest
import torch

from fluidgym_amd import _lib as L
from oracle import piso_oracle as O
from tests.helpers import NORMAL_FLUX_CASES, NORMAL_FLUX_DT, make_case, normal_flux_case, rel_err, slab_areas, with_normal_flux

pytestmark = pytest.mark.gpu

ASM_TOL = 1e-5       # tests/test_gpu_parity.py
SOLVE_TOL = 3e-5
F64 = torch.float64
NAMES = list(NORMAL_FLUX_CASES)
SCALAR_NAMES = [n for n in NAMES if "n_scalars" in NORMAL_FLUX_CASES[n]]
DT = NORMAL_FLUX_DT


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


@functools.lru_cache(maxsize=None)
def _assembly_reference(name):
    """Per env: (C, A, offs, rhs) of the velocity system and (Cs, As, rhs_s) of scalar channel 0 (or None); computed once, read only."""
    case = normal_flux_case(name)
    g = case.grid()
    out = []
    for b in range(case.B):
        dom = case.oracle_domain(b, g)
        C, A, offs = O.build_advection_matrix(dom, DT[b])
        vel = (C, A, offs, O.advection_rhs_velocity(dom, DT[b]))
        scal = None
        if case.scalar is not None:
            Cs, As, _ = O.build_advection_matrix(dom, DT[b], for_scalar=True, channel=0)
            scal = (Cs, As, O.advection_rhs_scalar(dom, DT[b])[0])
        out.append((vel, scal))
    return out


@functools.lru_cache(maxsize=None)
def _step_reference(name):
    """Per env: the oracle's split step from the case's state (intermediates + the stepped domain); computed once, read only."""
    case = normal_flux_case(name)
    g = case.grid()
    out = []
    for b in range(case.B):
        dom = case.oracle_domain(b, g)
        out.append((O.piso_split_step(dom, DT[b]), dom))
    return out


# ------------------------------------------------------------------------------------------------ fp32 library
@pytest.mark.parametrize("name", NAMES)
def test_advection_assembly_with_normal_flux(name):
    """k_adv_build: A, the off-diagonals and the velocity right-hand side (the u_b U_b terms of every fixed face)."""
    case = normal_flux_case(name)
    ns = case.native()
    ns.setup_advection(DT)
    d = case.dims
    A = _np(ns.buffer(0, (case.B,) + case.shape))
    off = _np(ns.buffer(1, (case.B, 2 * d) + case.shape))
    rhs = _np(ns.buffer(2, (case.B, d) + case.shape))
    ns.close()
    for b, ((_, A_ref, offs_ref, rhs_ref), _) in enumerate(_assembly_reference(name)):
        assert rel_err(A[b], A_ref) < ASM_TOL
        for f in range(2 * d):
            assert np.abs(off[b, f] - offs_ref[f]).max() < ASM_TOL * np.abs(A_ref).max()
        assert rel_err(rhs[b], rhs_ref) < ASM_TOL, (b, rel_err(rhs[b], rhs_ref))


@pytest.mark.parametrize("name", SCALAR_NAMES)
def test_scalar_assembly_and_solve_with_normal_flux(name):
    """The SCALAR instance of k_adv_build: Dirichlet faces (t_b U_b) and the Neumann face (the stored datum times U_b)."""
    case = normal_flux_case(name)
    ns = case.native()
    ns.setup_advection(DT, for_scalar=True, channel=0)
    A = _np(ns.buffer(0, (case.B,) + case.shape))
    rhs = _np(ns.buffer(2, (case.B * case.dims,) + case.shape))[: case.B]
    info = ns.solve_advection(for_scalar=True, tol=1e-7)
    assert all(i.converged for i in info)
    res = _np(ns.buffer(7, (case.B,) + case.shape))
    ns.close()
    for b, (_, (Cs, A_ref, rhs_ref)) in enumerate(_assembly_reference(name)):
        assert rel_err(A[b], A_ref) < ASM_TOL
        assert rel_err(rhs[b], rhs_ref) < ASM_TOL, (b, rel_err(rhs[b], rhs_ref))
        x_ref = O.solve_direct(Cs, rhs_ref.ravel()).reshape(case.shape)
        assert rel_err(res[b], x_ref) < SOLVE_TOL


@pytest.mark.parametrize("name", NAMES)
def test_piso_step_intermediates_with_normal_flux(name):
    """One split step from identical state: h, div (k_div's boundary fluxes on every fixed face), velocity, pressure and its mean."""
    case = normal_flux_case(name)
    ns = case.native()
    g = case.grid()
    d = case.dims
    ok, stats = ns.piso_step(DT, advection_tol=1e-7, pressure_tol=1e-7)
    torch.cuda.synchronize()
    vel = _np(ns.velocity)
    p = _np(ns.pressure)[:, 0]
    scal = None if case.scalar is None else _np(ns.scalar)
    h = _np(ns.buffer(4, (case.B, d) + case.shape))
    div = _np(ns.buffer(5, (case.B,) + case.shape))
    ns.close()
    area_max = max(float((g.det * g.Minv[..., a, a]).max()) for a in range(d))
    for b, (out, dom) in enumerate(_step_reference(name)):
        assert rel_err(h[b], out["h1"]) < SOLVE_TOL
        div_scale = max(np.abs(out["div1"]).max(), np.abs(out["h1"]).max() * area_max)
        assert np.abs(div[b] - out["div1"]).max() < SOLVE_TOL * div_scale
        assert rel_err(vel[b], dom.velocity) < SOLVE_TOL, (b, rel_err(vel[b], dom.velocity))
        assert rel_err(p[b], dom.pressure) < 10 * SOLVE_TOL
        assert abs(p[b].mean()) < 1e-5 * np.abs(p[b]).max()
        if scal is not None:
            assert rel_err(scal[b], dom.scalar) < SOLVE_TOL
    assert stats[1] >= 0 and stats[2] > 0


@pytest.mark.parametrize("name", ["2d_box", "3d_channel"])
def test_per_cell_viscosity_with_normal_flux(name):
    """The VISC instance of k_adv_build with a rough viscosity field (tests/test_gpu_sgs.py), through-flow on every fixed face."""
    case = normal_flux_case(name)
    dims = case.dims
    rng = np.random.default_rng(5)
    fields = [0.02 * (1.0 + 4.0 * rng.random(case.shape)) for _ in range(case.B)]       # 0.02 .. 0.1, rough
    ns = case.native()
    ns.set_viscosity_field(torch.as_tensor(np.stack(fields), dtype=torch.float32, device="cuda").contiguous())
    ns.set_advection_start(False)
    ns.setup_advection(DT)
    A = _np(ns.buffer(0, (case.B,) + case.shape))
    off = _np(ns.buffer(1, (case.B, 2 * dims) + case.shape))
    rhs = _np(ns.buffer(2, (case.B, dims) + case.shape))
    info = ns.solve_advection(tol=1e-7)
    assert all(i.converged for i in info)
    x = _np(ns.buffer(3, (case.B, dims) + case.shape))
    ns.close()
    g = case.grid()
    for b in range(case.B):
        dom = case.oracle_domain(b, g)
        A0 = _assembly_reference(name)[b][0][1]
        dom.viscosity_field = fields[b]
        C, A_ref, offs = O.build_advection_matrix(dom, DT[b])
        assert rel_err(A_ref, A0) > 1e-2                       # the field matters
        assert rel_err(A[b], A_ref) < 1e-5
        for f in range(2 * dims):
            assert np.abs(off[b, f] - offs[f]).max() < 1e-5 * np.abs(A_ref).max()
        rhs_ref = O.advection_rhs_velocity(dom, DT[b])
        assert rel_err(rhs[b], rhs_ref) < 2e-5
        for comp in range(dims):
            assert rel_err(x[b, comp], O.solve_direct(C, rhs_ref[comp].ravel()).reshape(case.shape)) < 3e-5


@pytest.mark.parametrize("name", ["2d_box", "3d_box_vec1"])
def test_make_divergence_free_with_normal_flux(name):
    case = normal_flux_case(name)
    ns = case.native()
    g = case.grid()
    ns.make_divergence_free(tol=1e-7)
    torch.cuda.synchronize()
    vel = _np(ns.velocity)
    ns.close()
    for b in range(case.B):
        dom = case.oracle_domain(b, g)
        O.make_divergence_free(dom)
        assert rel_err(vel[b], dom.velocity) < SOLVE_TOL, (b, rel_err(vel[b], dom.velocity))


# ------------------------------------------------------------------------------------------------ fp64 library
@pytest.mark.parametrize("name", NAMES)
def test_fp64_assembly_and_solves_with_normal_flux(name):
    """The same kernel source in doubles (tests/test_gpu_f64.py): assembly to machine precision, solves to 1e-12."""
    case = normal_flux_case(name)
    ns = case.native(dtype=F64)
    assert ns.velocity.dtype == F64 and ns.f64
    shape = (case.B, case.dims) + case.shape
    ns.set_advection_start(False)
    ns.setup_advection(DT)
    A = _np(ns.buffer(L.FG_BUF_A, (case.B,) + case.shape))
    rhs = _np(ns.buffer(L.FG_BUF_ADV_RHS, shape))
    info = ns.solve_advection(tol=1e-13)
    assert all(i.converged and i.is_finite for i in info)
    x = _np(ns.buffer(L.FG_BUF_VEL_RESULT, shape))
    rhs_s = None
    if case.scalar is not None:
        ns.setup_advection(DT, for_scalar=True, channel=0)
        A_s = _np(ns.buffer(L.FG_BUF_A, (case.B,) + case.shape))
        rhs_s = _np(ns.buffer(L.FG_BUF_ADV_RHS, (case.B * case.dims,) + case.shape))[: case.B]
    ns.close()
    for b, ((C, A_ref, _, rhs_ref), scal) in enumerate(_assembly_reference(name)):
        ex = max(rel_err(x[b, comp], O.solve_direct(C, rhs_ref[comp].ravel()).reshape(case.shape)) for comp in range(case.dims))
        print(f"F64_ERR normal-flux assembly {name} env {b}: A {rel_err(A[b], A_ref):.1e} rhs {rel_err(rhs[b], rhs_ref):.1e} solve {ex:.1e}")
        assert rel_err(A[b], A_ref) < 1e-14
        assert rel_err(rhs[b], rhs_ref) < 1e-14
        assert ex < 1e-12
        if scal is not None:
            print(f"F64_ERR normal-flux scalar assembly {name} env {b}: A {rel_err(A_s[b], scal[1]):.1e} rhs {rel_err(rhs_s[b], scal[2]):.1e}")
            assert rel_err(A_s[b], scal[1]) < 1e-14
            assert rel_err(rhs_s[b], scal[2]) < 1e-14


@pytest.mark.parametrize("name", NAMES)
def test_fp64_piso_step_with_normal_flux(name):
    case = normal_flux_case(name)
    ns = case.native(dtype=F64)
    ok, stats = ns.piso_step(DT, advection_tol=1e-13, pressure_tol=1e-13, max_iterations=20000)
    assert ok, stats
    vel, pres = _np(ns.velocity), _np(ns.pressure)
    scal = None if case.scalar is None else _np(ns.scalar)
    ns.close()
    for b, (_, dom) in enumerate(_step_reference(name)):
        p = pres[b, 0]
        eu, ep = rel_err(vel[b], dom.velocity), rel_err(p - p.mean(), dom.pressure - dom.pressure.mean())
        es = 0.0 if scal is None else rel_err(scal[b], dom.scalar)
        print(f"F64_ERR normal-flux step {name} env {b}: velocity {eu:.1e} pressure {ep:.1e} scalar {es:.1e} iterations {stats}")
        assert eu < 1e-10, (b, stats)
        assert ep < 1e-9
        assert es < 1e-9


# ------------------------------------------------------------------------------------------------ the fused pressure path
def test_fused_pressure_path_with_normal_flux(monkeypatch):
    """k_fcg_div_fwd (csrc/fg_fftcg.hip) computes the pressure right-hand side's boundary fluxes itself: through-flow on all four
    faces of the channel case of tests/test_gpu_fused_cg.py, the fused solver against the five kernels and the oracle at that
    test's gates -- and the handle must say that the fused row kernels ran (FG_CG_FUSED=1 on a fast-transform grid), not k_div."""
    from tests.test_gpu_fused_cg import _channel_case

    case = with_normal_flux(_channel_case((64, 24)), 5)
    g = case.grid()
    dt = [0.02, 0.0, 0.03]
    res = {}
    for mode in ("1", "0", "1p"):
        monkeypatch.setenv("FG_CG_FUSED", mode[0])
        ns = case.native()
        cfg = ns.config_dump()
        # fg_fcg_ok: the switch, the FD preconditioner with a fast x transform, 2-D, fixed y -- else fg_launch_div falls back to k_div
        assert cfg["FG_CG_FUSED"] == int(mode[0]) and cfg["fd_preconditioner"] == 1 and cfg["fast_transform_x"] != 0
        assert ns.has_fd and ns.default_method == L.FG_SOLVER_FDCG and ns.dims == 2
        if mode == "1p":
            ns.profile_enable(True)      # a third run that counts launches: the fused kernels ran, and give the unprofiled run's step
        v0 = ns.velocity.clone()
        ok, stats = ns.piso_step(dt, advection_tol=1e-7, pressure_tol=1e-7)
        torch.cuda.synchronize()
        assert ok, stats
        res[mode] = (_np(ns.velocity), _np(ns.pressure), stats)
        assert torch.equal(ns.velocity[1], v0[1])     # masked env
        if mode == "1p":
            prof = ns.profile_read()
            ns.profile_enable(False)
            assert prof["k_fcg_inv_apply"]["launches"] > 0, prof["k_fcg_inv_apply"]
        ns.close()
    assert rel_err(res["1p"][0], res["1"][0]) < 1e-6
    for b in (0, 2):
        dom = case.oracle_domain(b, g)
        assert abs(O.boundary_flux_balance(dom)) < 1e-12
        O.piso_split_step(dom, dt[b])
        for mode in ("1", "0"):
            u, p, _ = res[mode]
            assert rel_err(u[b], dom.velocity) < 3e-5, (mode, b, rel_err(u[b], dom.velocity))
            assert abs(p[b].mean()) < 1e-5 * np.abs(p[b]).max(), (mode, b, p[b].mean())
            assert rel_err(p[b, 0], dom.pressure) < 2e-4, (mode, b)
        assert rel_err(res["1"][0][b], res["0"][0][b]) < 5e-5
        assert rel_err(res["1"][1][b], res["0"][1][b]) < 5e-5


# ------------------------------------------------------------------------------------------------ reductions, face by face
# closed on every axis; more than 64 entries along the lane axis and more than 16 rows on every face, so every loop of the slab
# scans wraps.  nx % 4 == 0: the row kernel (k_max_velocity_rows); otherwise the element-wise one.
REDUCTION_SHAPES = [(68, 66, 19), (66, 65, 18), (68, 66), (66, 65)]


@functools.lru_cache(maxsize=None)
def _reduction_case(n):
    """B = 2 d envs of a box closed on every axis with small fields (1e-3) that both sides hold exactly (fp32 values), and its grid."""
    dims = len(n)
    case = make_case(dims=dims, n=n, fixed_axes=tuple(range(dims)), B=2 * dims, seed=41, vel_scale=1e-3, wall_motion=1e-3)
    case.velocity = case.velocity.astype(np.float32).astype(np.float64)
    case.bvel = {f: v.astype(np.float32).astype(np.float64) for f, v in case.bvel.items()}
    return case, case.grid()


def _with_bvel(case, bvel):
    import copy

    c = copy.copy(case)
    c.bvel = bvel
    return c


@pytest.mark.parametrize("n", REDUCTION_SHAPES, ids=lambda n: "x".join(map(str, n)))
def test_max_velocity_finds_a_maximum_on_every_face(n):
    """k_max_velocity / k_max_velocity_rows: env b carries one large entry on face b, at a random slab position, in component
    (b + 1) % d -- the normal one on some faces, a tangential one on others.  Bound: the kernel's one fp32 multiply by 1/h (and the
    rounding of 1/h itself) on inputs both sides share, ~1.2e-7; 1e-6 is that with margin."""
    base, g = _reduction_case(n)
    d = base.dims
    rng = np.random.default_rng(7)
    bvel = {f: v.copy() for f, v in base.bvel.items()}
    where = {}
    for b in range(base.B):
        slab = bvel[b][b, (b + 1) % d]
        where[b] = tuple(int(rng.integers(s)) for s in slab.shape)
        slab[where[b]] = 5.0
    case = _with_bvel(base, bvel)
    ns = case.native()
    mv = _np(ns.max_velocity())
    _, mv_diag = ns.step_diagnostics()
    ns.close()
    for b in range(case.B):
        ref = O.max_velocity(case.oracle_domain(b, g))
        # the oracle's maximum lies on that face: without that one boundary value it is far smaller
        assert O.max_velocity(base.oracle_domain(b, g)) < 0.1 * ref
        assert abs(mv[b] - ref) < 1e-6 * ref, (b, where[b], mv[b], ref)
        assert abs(float(mv_diag[b]) - ref) < 1e-6 * ref, (b, where[b], mv_diag[b], ref)


@pytest.mark.parametrize("n", REDUCTION_SHAPES, ids=lambda n: "x".join(map(str, n)))
def test_flux_balance_weighs_and_signs_every_face(n):
    """fg_flux_balance_block: balanced random through-flow on every face (the control) and, in env b, an excess of 0.37 over a random
    half of face b.  Bound: the kernel rounds two fp32 products per term (area, then value times area) and sums in doubles, 1.2e-7 of
    sum |u_n| area; the gate is four times that."""
    base, g = _reduction_case(n)
    base = with_normal_flux(_with_bvel(base, {f: v.copy() for f, v in base.bvel.items()}), 9)
    base.bvel = {f: v.astype(np.float32).astype(np.float64) for f, v in base.bvel.items()}
    d = base.dims
    rng = np.random.default_rng(8)
    bvel = {f: v.copy() for f, v in base.bvel.items()}
    excess = {}
    for b in range(base.B):
        half = rng.random(bvel[b][b, b >> 1].shape) < 0.5
        bvel[b][b, b >> 1] += np.float32(0.37) * half
        excess[b] = float((np.float64(np.float32(0.37)) * half * slab_areas(base, b)).sum())
    bvel = {f: v.astype(np.float32).astype(np.float64) for f, v in bvel.items()}
    got = {}
    for key, case in (("control", base), ("excess", _with_bvel(base, bvel))):
        ns = case.native()
        fb = _np(ns.boundary_flux_balance())
        fb_diag, _ = ns.step_diagnostics()
        ns.close()
        got[key] = (case, fb, np.asarray(fb_diag, np.float64))
    for b in range(base.B):
        for key in ("control", "excess"):
            case, fb, fb_diag = got[key]
            bound = 5e-7 * sum(float((np.abs(case.bvel[f][b, f >> 1]) * slab_areas(case, f)).sum()) for f in case.fixed_faces)
            ref = O.boundary_flux_balance(case.oracle_domain(b, g))
            assert abs(fb[b] - ref) < bound, (key, b, fb[b], ref, bound)
            assert abs(fb_diag[b] - ref) < bound, (key, b, fb_diag[b], ref, bound)
            if key == "control":
                assert abs(ref) < bound and abs(fb[b]) < bound and abs(fb_diag[b]) < bound
        # an excess on a lower face lowers the balance, one on an upper face raises it -- by the excess's own flux
        fb = got["excess"][1]
        assert excess[b] > 100 * bound
        assert (fb[b] > 0.5 * excess[b]) if (b & 1) else (fb[b] < -0.5 * excess[b]), (b, fb[b], excess[b])
        assert abs(abs(fb[b]) - excess[b]) < 3 * bound      # (the control's own residual, the excess's fp32 rounding, the kernel's error)
