"""One viscosity / scalar diffusivity per env of a batch (``fg_set_viscosity_batch``, ``fg_set_scalar_viscosity_batch``,
``fg_mb_set_viscosity_batch``, ``fg_mb_wall_forces_batch``): every env of a heterogeneous batch against the oracle run at that env's
own values, at the bounds the homogeneous tests hold; a uniform array against the scalar path bit for bit."""
import numpy as np
import pytest
import torch

import helpers_mb as H
from oracle import piso_oracle as O
from tests.helpers import make_case, rel_err

pytestmark = pytest.mark.gpu
F64 = torch.float64
NU_B = (0.02, 0.05, 0.1, 0.2)
KAPPA_B = (0.15, 0.01, 0.06, 0.03)
ASM_TOL, SOLVE_TOL = 1e-5, 3e-5      # tests/test_gpu_parity.py: test_advection_assembly, test_full_piso_step_intermediates
CASES = {
    "2d_walls_y": dict(dims=2, n=(32, 12), fixed_axes=(1,)),
    "2d_periodic": dict(dims=2, n=(32, 16), fixed_axes=()),
    "3d_channel": dict(dims=3, n=(16, 10, 8), fixed_axes=(1,)),
    "3d_periodic": dict(dims=3, n=(16, 8, 8), fixed_axes=()),
}


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _wall_refined(case, ratio):
    """The y widths replaced by a two-sided geometric wall refinement (largest / smallest width = ratio)."""
    ny = len(case.widths[1])
    half = ny // 2
    g = ratio ** (1.0 / max(half - 1, 1))
    w = np.concatenate([g ** np.arange(half), g ** np.arange(ny - half)[::-1]])
    w = (w / w.sum()).astype(np.float32)
    case.widths[1] = w
    case.edges[1] = np.concatenate([[0.0], np.cumsum(w.astype(np.float64))])
    return case


def _install(ns, nu_B, kappa_B=None):
    ns.set_viscosity(torch.tensor(nu_B, dtype=torch.float64))
    if kappa_B is not None:
        ns.set_scalar_viscosity(0, torch.tensor(kappa_B, dtype=torch.float64))
    assert ns.viscosity_B is not None and ns.viscosity_B.is_cuda and ns.viscosity_B.dtype == ns.dtype


def _oracle(case, b, g, nu_B, kappa_B):
    dom = case.oracle_domain(b, g)
    dom.viscosity = float(nu_B[b])
    if kappa_B is not None:
        dom.scalar_viscosity = [float(kappa_B[b])]
    return dom


@pytest.mark.parametrize("dtype", [torch.float32, F64])
@pytest.mark.parametrize("name", list(CASES))
def test_assembly_and_solves_per_env(name, dtype):
    """A, off-diagonals and right-hand side of the velocity and the scalar system of each env against the oracle at that env's own
    nu / kappa; fp64 also the solves."""
    case = make_case(**CASES[name], B=4, seed=3, with_source=True, n_scalars=1)
    ns = case.native(dtype=dtype)
    _install(ns, NU_B, KAPPA_B)
    g, d = case.grid(), case.dims
    dt = [0.05, 0.02, 0.04, 0.03]
    asm = 1e-14 if dtype == F64 else ASM_TOL
    for for_scalar in (False, True):
        ns.setup_advection(dt, for_scalar=for_scalar, channel=0)
        nc = 1 if for_scalar else d
        A = _np(ns.buffer(0, (case.B,) + case.shape))
        off = _np(ns.buffer(1, (case.B, 2 * d) + case.shape))
        rhs = _np(ns.buffer(2, (case.B * d,) + case.shape))[: case.B * nc].reshape((case.B, nc) + case.shape)
        x = None
        if dtype == F64:
            info = ns.solve_advection(for_scalar=for_scalar, tol=1e-14, max_iterations=20000)
            assert all(i.converged for i in info)
            x = _np(ns.buffer(7, (case.B,) + case.shape)).reshape((case.B, 1) + case.shape) if for_scalar else \
                _np(ns.buffer(3, (case.B, d) + case.shape))
        for b in range(case.B):
            dom = _oracle(case, b, g, NU_B, KAPPA_B)
            C, A_ref, offs_ref = O.build_advection_matrix(dom, dt[b], for_scalar=for_scalar, channel=0)
            rhs_ref = O.advection_rhs_scalar(dom, dt[b])[:1] if for_scalar else O.advection_rhs_velocity(dom, dt[b])
            errs = [rel_err(A[b], A_ref), max(np.abs(off[b, f] - offs_ref[f]).max() for f in range(2 * d)) / np.abs(A_ref).max(),
                    rel_err(rhs[b], np.asarray(rhs_ref))]
            print(f"PER_ENV_ASM {name} {dtype} scalar={for_scalar} env {b}: A {errs[0]:.1e} off {errs[1]:.1e} rhs {errs[2]:.1e}")
            assert max(errs) < asm, (b, for_scalar, errs)
            if x is not None:
                for c in range(nc):
                    x_ref = O.solve_direct(C, np.asarray(rhs_ref)[c].ravel()).reshape(case.shape)
                    assert rel_err(x[b, c], x_ref) < 1e-12, (b, for_scalar, c)
    ns.close()


@pytest.mark.parametrize("dtype", [torch.float32, F64])
@pytest.mark.parametrize("name", ["2d_walls_y", "3d_channel"])
def test_whole_piso_step_per_env(name, dtype):
    """One split step (scalar, predictor, two correctors) of a heterogeneous batch: fp64 to the bounds of
    test_fp64_piso_step_matches_the_oracle_to_1e9, fp32 to those of test_full_piso_step_intermediates.  Power: the oracle's own
    results for two entries of nu_B differ by at least 100 times the bound, so a kernel that ignored the array cannot pass."""
    f64 = dtype == F64
    case = make_case(**CASES[name], B=4, seed=21, with_source=True, vel_scale=0.3, n_scalars=1)
    ns = case.native(dtype=dtype)
    _install(ns, NU_B, KAPPA_B)
    g, dt = case.grid(), 0.03
    # (fp32 solves to 1e-8: at 1e-7 env 3 -- nu 0.2, the stiffest matrix -- lands at velocity 3.07e-05 against the bound 3e-05 with or
    #  without the array, the homogeneous batch at nu 0.2 giving the same figure to three digits; at 1e-8 both give 9.1e-07)
    tol = 1e-13 if f64 else 1e-8
    ok, stats = ns.piso_step(dt, advection_tol=tol, pressure_tol=tol, max_iterations=20000)
    assert ok, stats
    bu, bp, bs = (1e-10, 1e-9, 1e-9) if f64 else (SOLVE_TOL, 10 * SOLVE_TOL, SOLVE_TOL)
    for b in range(case.B):
        dom = _oracle(case, b, g, NU_B, KAPPA_B)
        O.piso_split_step(dom, dt)
        p = _np(ns.pressure[b, 0])
        eu = rel_err(_np(ns.velocity[b]), dom.velocity)
        ep = rel_err(p - p.mean(), dom.pressure - dom.pressure.mean())
        es = rel_err(_np(ns.scalar[b]), dom.scalar)
        print(f"PER_ENV_STEP {name} {dtype} env {b}: velocity {eu:.1e} pressure {ep:.1e} scalar {es:.1e} iterations {stats}")
        assert eu < bu and ep < bp and es < bs, (b, eu, ep, es)
    if not f64 and name == "3d_channel":
        # control for the tolerance above: at 1e-7 (what test_full_piso_step_intermediates solves to) env 3 of the mixed batch and the
        # same env of a HOMOGENEOUS batch at nu 0.2 through the scalar entry land on the same error -- the solver tolerance, not the array
        errs = []
        for per_env in (True, False):
            c7 = make_case(**CASES[name], B=4, seed=21, with_source=True, vel_scale=0.3, n_scalars=1)
            if not per_env:
                c7.nu, c7.kappa = NU_B[3], [KAPPA_B[3]]
            n7 = c7.native()
            if per_env:
                _install(n7, NU_B, KAPPA_B)
            assert n7.piso_step(dt, advection_tol=1e-7, pressure_tol=1e-7, max_iterations=20000)[0]
            dom = _oracle(case, 3, g, NU_B, KAPPA_B)
            O.piso_split_step(dom, dt)
            errs.append(rel_err(_np(n7.velocity[3]), dom.velocity))
            n7.close()
        print(f"PER_ENV_STEP control at 1e-7, env 3: mixed {errs[0]:.3e} homogeneous {errs[1]:.3e}")
        assert abs(errs[0] - errs[1]) < 0.01 * errs[1], errs
    # power: env 0's state stepped with nu_B[0] and with nu_B[3]
    a, c = _oracle(case, 0, g, NU_B, KAPPA_B), _oracle(case, 0, g, NU_B[::-1], KAPPA_B[::-1])
    O.piso_split_step(a, dt), O.piso_split_step(c, dt)
    assert rel_err(c.velocity, a.velocity) > 100 * bu and rel_err(c.scalar, a.scalar) > 100 * bs
    ns.close()


def _three_steps(case, per_env, prepare=None, buoyancy=False):
    ns = case.native()
    if prepare:
        prepare(ns)
    if per_env:
        _install(ns, [case.nu] * case.B, [case.kappa[0]] * case.B if case.kappa else None)
    kw = dict(buoyancy_axis=1, buoyancy_factor=1.0) if buoyancy else {}
    for _ in range(3):
        ns.piso_step(0.03, advection_tol=1e-6, pressure_tol=1e-6, **kw)
    torch.cuda.synchronize()
    out = (ns.velocity.clone(), ns.pressure.clone(), None if ns.scalar is None else ns.scalar.clone())
    ns.close()
    return out


def _same(a, b):
    for x, y in zip(a, b):
        assert (x is None and y is None) or torch.equal(x, y)


def test_uniform_array_is_the_scalar_path_default_forms():
    for kw in (CASES["2d_walls_y"], CASES["3d_channel"]):
        case = make_case(**kw, B=3, seed=5, with_source=True, vel_scale=0.3, n_scalars=1)
        _same(_three_steps(case, False), _three_steps(case, True))


def test_uniform_array_is_the_scalar_path_helmholtz_pair():
    """RBC-shaped: periodic uniform x (a multiple of 64: the row form and the pair factorisation ahead of the solves), walls in y."""
    case = make_case(dims=2, n=(64, 32), fixed_axes=(1,), B=3, seed=7, stretch=0.0, vel_scale=0.3, n_scalars=1, wall_motion=0.0)
    case.source = np.zeros_like(case.velocity)

    def prep(ns):
        assert ns.has_helmholtz
        ns.set_advection_preconditioner(3)
    _same(_three_steps(case, False, prep, buoyancy=True), _three_steps(case, True, prep, buoyancy=True))


def test_uniform_array_is_the_scalar_path_jacobi():
    case = make_case(dims=2, n=(64, 32), fixed_axes=(1,), B=3, seed=8, stretch=0.0, vel_scale=0.3)
    _same(_three_steps(case, False, lambda ns: ns.set_advection_jacobi(True)),
          _three_steps(case, True, lambda ns: ns.set_advection_jacobi(True)))


def test_uniform_array_is_the_scalar_path_multiblock_cylinder():
    spec = H.cylinder_2d()
    out = []
    for per_env in (False, True):
        dom = spec.native(batch=2)
        if per_env:
            dom.set_viscosity([spec.nu, spec.nu])
            assert dom.viscosity_B is not None
        rng = np.random.default_rng(0)
        dom.velocity.copy_(torch.as_tensor(0.2 * rng.standard_normal(tuple(dom.velocity.shape)), dtype=torch.float32))
        dom.piso_step(0.02, advection_tol=1e-6, pressure_tol=1e-6, raise_on_failure=False)
        torch.cuda.synchronize()
        out.append((dom.velocity.clone(), dom.pressure.clone()))
        dom.close()
    _same(out[0], out[1])


def test_helmholtz_heterogeneous_and_values_rewritten_in_place():
    """Preconditioner forced (mode 3) on an RBC-shaped case; nu / kappa per env over the registry's Rayleigh range (Ra 8e4 .. 8e5 at
    Pr 0.7: nu = sqrt(Pr / Ra), kappa = 1 / sqrt(Ra Pr)).  Every env converges to the bound of tests/test_gpu_helmholtz.py (3e-5)
    against the direct solve at its own values; then the arrays are REWRITTEN IN PLACE (same addresses) and the next solves and a
    whole step follow the new values: a factor set made for the old ones must not be reused."""
    ra = np.array([8e4, 4e5, 8e5])
    nu_B, ka_B = np.sqrt(0.7 / ra), 1.0 / np.sqrt(ra * 0.7)
    case = _wall_refined(make_case(dims=2, n=(64, 32), fixed_axes=(1,), B=3, seed=4, vel_scale=0.3, stretch=0.0, n_scalars=1), ratio=10.0)
    ns = case.native()
    assert ns.has_helmholtz
    ns.set_advection_start(False)
    ns.set_advection_preconditioner(3)
    _install(ns, nu_B, ka_B)
    g, dt = case.grid(), 0.05

    def check(nu_now, ka_now):
        for for_scalar in (True, False):
            ns.setup_advection(dt, for_scalar=for_scalar, channel=0)
            info = ns.solve_advection(for_scalar=for_scalar, tol=1e-7)
            assert all(i.converged and i.is_finite for i in info), [i.final_residual for i in info]
            x = _np(ns.buffer(7, (case.B,) + case.shape))[:, None] if for_scalar else _np(ns.buffer(3, (case.B, 2) + case.shape))
            for b in range(case.B):
                dom = _oracle(case, b, g, nu_now, ka_now)
                C, _, _ = O.build_advection_matrix(dom, dt, for_scalar=for_scalar, channel=0)
                rhs = O.advection_rhs_scalar(dom, dt)[:1] if for_scalar else O.advection_rhs_velocity(dom, dt)
                for c in range(x.shape[1]):
                    x_ref = O.solve_direct(C, np.asarray(rhs)[c].ravel()).reshape(case.shape)
                    assert rel_err(x[b, c], x_ref) < 3e-5, (b, for_scalar, c)

    check(nu_B, ka_B)
    # a whole step (the pair factorisation ahead of the solves), then new values written into the SAME device arrays
    v0, s0 = ns.velocity.clone(), ns.scalar.clone()
    ns.piso_step(dt, advection_tol=1e-7, pressure_tol=1e-7)
    first = ns.velocity.clone()
    nu_2, ka_2 = nu_B[::-1].copy(), ka_B[::-1].copy()
    ns.viscosity_B.copy_(torch.as_tensor(nu_2, dtype=torch.float32))
    ns.scalar_viscosities_B[0].copy_(torch.as_tensor(ka_2, dtype=torch.float32))
    ns.velocity.copy_(v0), ns.scalar.copy_(s0)
    ns.pressure.zero_()
    ns.copy_velocity_result_from_blocks()
    check(nu_2, ka_2)
    ns.velocity.copy_(v0), ns.scalar.copy_(s0)
    ns.copy_velocity_result_from_blocks()
    ok, stats = ns.piso_step(dt, advection_tol=1e-8, pressure_tol=1e-8)      # (1e-7 leaves 3.07e-05 in env 0: solver tolerance)
    assert ok, stats
    for b in range(case.B):
        dom = _oracle(case, b, g, nu_2, ka_2)
        dom.velocity, dom.scalar = _np(v0[b]), _np(s0[b])
        O.piso_split_step(dom, dt)
        assert rel_err(_np(ns.velocity[b]), dom.velocity) < SOLVE_TOL, b
    assert not torch.equal(first[0], ns.velocity[0])
    ns.close()


def test_multiblock_cylinder_step_and_wall_forces_per_env():
    """fp64 build, the cylinder mesh, B = 3 at Re (100, 200, 400): one step against mb_oracle at each env's nu (bounds of
    tests/test_gpu_mb_f64.py), the wall forces against the tensor form of the reference's arithmetic (tests/test_forces.py holds it
    on the reference's vectors) with that env's nu."""
    from fluidgym_amd import _lib as L
    spec = H.cylinder_2d()
    d = spec.oracle()
    B, nu_B = 3, [1.0 / 100, 1.0 / 200, 1.0 / 400]
    dom = spec.native(batch=B, dtype=F64)
    with pytest.raises(ValueError):
        dom.set_viscosity([0.01, 0.0, 0.01])
    dom.set_viscosity(nu_B)
    rng = np.random.default_rng(3)
    u0 = 0.2 * rng.standard_normal((B, d.d, d.N))
    dom.velocity.copy_(torch.as_tensor(u0, dtype=F64))
    dt = 0.02
    its = dom.piso_step(dt, advection_tol=1e-13, pressure_tol=1e-13, max_iterations=20000, raise_on_failure=False)
    assert its[0] > 0 and its[1] > 0
    A = dom.buffer(L.FG_MB_BUF_A).view(B, -1).cpu().numpy()
    rhs = dom.buffer(L.FG_MB_BUF_RHS).view(B, d.d, -1).cpu().numpy()
    refs = []
    for b in range(B):
        d.nu = nu_B[b]
        trace = {}
        u_ref, p_ref = d.piso_step(u0[b], np.zeros(d.N), dt, trace=trace)
        refs.append(u_ref)
        p = _np(dom.pressure[b])
        errs = {"A": rel_err(A[b], trace["C"][0]), "rhs": rel_err(rhs[b], trace["rhs"]), "velocity": rel_err(_np(dom.velocity[b]), u_ref),
                "pressure": rel_err(p - p.mean(), p_ref - p_ref.mean())}
        print(f"PER_ENV_MB env {b}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
        assert errs["A"] < 1e-11 and errs["rhs"] < 1e-11 and errs["velocity"] < 1e-8 and errs["pressure"] < 1e-7, errs
    assert rel_err(refs[2], refs[0]) > 100 * 1e-8      # power: the oracle's envs differ far beyond the bound
    # wall forces: the cylinder's own ring, built as the env builds it, through WallRing.forces with a [B] tensor (one launch of
    # fg_mb_wall_forces_batch) against the tensor form of the reference's arithmetic at each env's nu
    from fluidgym_amd.envs.cylinder_grid import BOTTOM, LEFT, RIGHT, TOP
    from fluidgym_amd.envs.forces import WallRing

    ring = WallRing(dom, [(LEFT, "+x", False), (TOP, "-y", False), (RIGHT, "-x", True), (BOTTOM, "+y", True)])
    f = ring.forces(dom, torch.tensor(nu_B, dtype=F64)).cpu()
    assert f.shape == (B, 2)
    for b in range(B):
        ref = ring.forces_tensor_form(dom, nu_B[b])[b].cpu()
        assert np.allclose(f[b].numpy(), ref.numpy(), rtol=1e-10, atol=1e-13), (b, f[b], ref)
    assert not np.allclose(f[2].numpy(), ring.forces_tensor_form(dom, nu_B[0])[2].cpu().numpy(), rtol=1e-3)
    # the library's own check of an installed array (the Python layer refuses a non-positive entry before it gets there)
    import ctypes
    bad = torch.tensor([0.01, 0.0, 0.01], dtype=F64, device="cuda")
    assert dom.lib.fg_mb_set_viscosity_batch(dom.handle, ctypes.c_void_p(bad.data_ptr())) == -1      # FG_ERR_INVALID_ARG
    assert b"positive" in dom.lib.fg_last_error()
    dom.close()


# ---- envs ------------------------------------------------------------------------------------------------------------------
ENV_CASES = {
    "RBC2D-easy-v0": ("rayleigh_number", [8e4, 4e5, 8e5], {}),
    "CylinderJet2D-easy-v0": ("reynolds_number", [100.0, 150.0, 200.0], dict(initial_domain_steps=20)),
}


def env_run(env_id, key, values, kw, perturb_others_of=None):
    """Two env steps after reset(seed=0) of a 3-env batch under a fixed action; ``perturb_others_of = b``: noise on the fields of
    the envs other than b right after the reset (the sensitivity measurement)."""
    import fluidgym_amd

    env = fluidgym_amd.make(env_id, num_envs=3, **{key: values}, **kw)
    env.reset(seed=0)
    if perturb_others_of is not None:
        g = torch.Generator().manual_seed(5)
        others = [o for o in range(3) if o != perturb_others_of]
        fields = [env._domain.velocity, env._domain.pressure] if hasattr(env._domain, "n_cells") else \
                 [env._block.velocity, env._block.passiveScalar]
        for fld in fields:
            for o in others:
                fld[o] += (0.05 * torch.randn(fld[o].shape, generator=g)).to(fld.device, fld.dtype)
    a = torch.zeros(env._zero_action.shape, device="cuda")
    for b, v in enumerate((0.3, -0.2, 0.5)):
        a[b] = v
    for _ in range(2):
        obs, reward, _, _, info = env.step(a)
    torch.cuda.synchronize()
    out = {k: v.detach().double().cpu() for k, v in obs.items()}
    out["reward"] = reward.detach().double().cpu()
    return out


@pytest.mark.parametrize("env_id", list(ENV_CASES))
def test_env_of_a_mixed_batch_is_the_env_of_the_homogeneous_batch(env_id):
    """Env b of ``make(env_id, num_envs=3, <parameter>=[three values])`` against env b of the homogeneous 3-env batch at value b: same
    batch size, index and seed, so the same random draws; two env steps after ``reset(seed=0)``.

    Whether a converged env is frozen: the CG and BiCGStab kernels skip a system whose flag is set (fg_cg.h: "skipped by that kernel
    and, through flags, by everything launched after it"; fg_bicg.h: ``f != 0``), and the Jacobi kernels return for an env whose
    systems are all flagged (fg_jacobi.hip), but the sweeps run PLANNED passes whose length comes from the handle's history of the
    whole batch (jac_hist: one record per solve kind, not per env), so the flags alone do not settle it.  The sensitivity was
    therefore measured on the parent commit: env b of a homogeneous batch against the same batch with N(0, 0.05) noise on the OTHER
    envs' fields after the reset (which moved those envs' observations by 2e-2 .. 2e-1), for each of the three values and each b.
    Measured: 0.0 exactly for every observation and the reward, RBC2D-easy-v0 and CylinderJet2D-easy-v0 alike; the doubled bound is
    0.0 -- the comparison is ``torch.equal``."""
    key, values, kw = ENV_CASES[env_id]
    mixed = env_run(env_id, key, values, kw)
    worst = {}
    homog = []
    for b in range(3):
        h = env_run(env_id, key, values[b], kw)
        homog.append(h)
        for k in mixed:
            worst[k] = max(worst.get(k, 0.0), float((mixed[k][b] - h[k][b]).abs().max()))
    print(f"PER_ENV_ENV {env_id}: " + " ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    for b in range(3):
        for k in mixed:
            assert torch.equal(mixed[k][b], homog[b][k][b]), (b, k, worst[k])
    # power: the same env index at another parameter value is a different trajectory
    for k in mixed:
        far = float((homog[0][k][2] - homog[2][k][2]).abs().max())
        print(f"PER_ENV_ENV {env_id} {k}: env 2 at value 0 against value 2 differs by {far:.2e}")
        assert far > 0.0, k


def test_channel_env_native_glue_uses_each_envs_own_shear_coefficient():
    """A mixed ChannelJet2D batch stepping through the native glue (fg_envglue_channel_observe_batch): the reported wall shear is the
    tensor form's with env b's own nu / (hy / 2), to the fp32 rounding of a different summation order."""
    import fluidgym_amd

    re_B = [100.0, 200.0, 400.0]
    env = fluidgym_amd.make("ChannelJet2D-v0", num_envs=3, reynolds_number=re_B, resolution_x=64, resolution_y=32)
    env.reset(seed=0)
    assert env._native_glue and env.heterogeneous
    a = torch.tensor([[0.3], [-0.2], [0.5]], device="cuda")
    _, reward, _, _, info = env.step(a)
    cross, shear = env._metrics_now()
    assert torch.allclose(info["wall_shear"], shear, rtol=1e-5, atol=1e-8), (info["wall_shear"], shear)
    assert torch.allclose(reward, -(shear + env._lift_penalty * cross), rtol=1e-5, atol=1e-8)
    u = env._block.velocity
    raw = (u[:, 0, 0, :].mean(dim=1) + u[:, 0, -1, :].mean(dim=1)) / (0.5 * env._hy)
    for b in range(3):
        assert float(info["wall_shear"][b]) == pytest.approx(float(raw[b]) / re_B[b], rel=1e-4)
