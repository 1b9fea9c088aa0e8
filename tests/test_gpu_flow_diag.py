"""Velocity-gradient diagnostics on the GPU (``fg_flow_diagnostic`` / ``fg_mb_flow_diagnostic``, csrc/fg_flowdiag.hip) in both
libraries: the gradient against the fp64 restatements of ``tests/flow_diag_ref.py`` to ``8 eps A`` in every cell of every env, the
derived kinds against their formulas in doubles from the GPU's own gradient, the Smagorinsky kernel as a second witness of the
strain norm, a rigid rotation as a case independent of both restatements, the state the calls must not touch, the argument errors,
and the env accessors.  The bounds are derived in ``flow_diag_ref`` (in units of the build's machine epsilon), not measured."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from fluidgym_amd import _lib as L
from tests import flow_diag_ref as R
from tests import helpers_mb as H
from tests.helpers import make_case, with_normal_flux

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float64]
SINGLE = [(2, (16, 12), (1,)), (2, (12, 10), (0, 1)), (3, (8, 6, 5), (1,)), (3, (6, 5, 4), (0, 1, 2)), (2, (12, 8), ()),
          (2, (70, 9), (1,)), (3, (66, 5, 3), (1,))]          # the last two cross the 64-cell tile edge in x and the 4-row chunk in y
MESHES = {"split_rotated_channel": H.split_rotated_channel, "skewed_pair": H.skewed_pair, "twisted_ring": H.twisted_ring,
          "skewed_pair_3d": H.skewed_pair_3d, "cylinder_3d_small": H.cylinder_3d_small, "cylinder_2d": lambda: H.cylinder_2d(res=8),
          "airfoil": lambda: H.airfoil_spec(div=4)}
C_SMAG = 0.17


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _eps(dtype):
    return float(torch.finfo(dtype).eps)


def _check_all_kinds(out, refs, d, eps, what):
    """``out[kind] [B, K, ...]`` of the GPU against ``refs[b] = (g, A)``; returns nothing, asserts everything."""
    for b, (g, A) in enumerate(refs):
        gpu_g = out[R.GRADIENT][b].reshape(g.shape)
        R.check_gradient(gpu_g, g, A, eps, f"{what} env {b}")
        for kind in R.KINDS[1:]:
            assert out[kind].shape[1] == R.channels(d, kind)
            R.check_derived(kind, out[kind][b], gpu_g, eps, f"{what} env {b}")


# ------------------------------------------------------------------------------------------------ single-block
@functools.lru_cache(maxsize=None)
def _single(idx, normal_flux=False):
    """``normal_flux``: a non-zero wall-normal wall value (the wall gradient du_n/dn is then not the gradient towards zero), set
    BEFORE the rounding of ``exact_case`` so that the inputs stay exactly representable."""
    dims, n, fixed_axes = SINGLE[idx]
    case = make_case(dims=dims, n=n, fixed_axes=fixed_axes, B=2, seed=7, nu=0.02, vel_scale=0.6)
    if normal_flux:
        case = with_normal_flux(case, 5)
    case = R.exact_case(case)
    grid = case.grid()
    refs = [R.single_block_gradient(case.oracle_domain(b, grid)) for b in range(case.B)]
    u_max = max([np.abs(case.velocity).max()] + [np.abs(v).max() for v in case.bvel.values()])
    for g, _ in refs:
        R.assert_not_trivial(g, u_max, max(float(w.max()) for w in case.widths))
    return case, grid, refs


def _single_state(ns):
    return [ns.velocity.clone(), ns.pressure.clone()] + [ns.bvel[f].clone() for f in sorted(ns.bvel)]


# (the normal_flux=False legs keep the ids they had before the parameter existed; the periodic grid has no wall, so no True leg)
SINGLE_LEGS = [(i, nf) for nf in (False, True) for i, s in enumerate(SINGLE) if s[2] or not nf]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("idx,normal_flux", SINGLE_LEGS,
                         ids=["x".join(map(str, SINGLE[i][1])) + "-fixed" + "".join(map(str, SINGLE[i][2])) + ("-normal_flux" if nf else "")
                              for i, nf in SINGLE_LEGS])
def test_single_block_kinds_against_the_oracle_gradient(idx, normal_flux, dtype):
    case, grid, refs = _single(idx, normal_flux)
    d, eps = case.dims, _eps(dtype)
    ns = case.native(dtype=dtype)
    ns.pressure.copy_(torch.randn(ns.pressure.shape, dtype=dtype, device=ns.device))
    before = _single_state(ns)
    out = {kind: _np(ns.flow_diagnostic(kind)) for kind in R.KINDS}
    nu_t = _np(ns.sgs_smagorinsky(C_SMAG))
    after = _single_state(ns)
    ns.close()
    assert all(torch.equal(a, b) for a, b in zip(before, after))      # velocity, pressure and boundary arrays: bit-identical
    for kind in R.KINDS:
        assert out[kind].shape == (case.B, R.channels(d, kind)) + case.shape
    _check_all_kinds(out, refs, d, eps, f"single {SINGLE[idx][1]}")
    # second witness: the Smagorinsky kernel's own stencil, nu_t = C Delta^2 |S| with Delta^2 as oracle.sgs_smagorinsky forms it
    delta = np.max(np.stack([np.sum(grid.M[..., :, a] ** 2, axis=-1) for a in range(d)]), axis=0)
    want = C_SMAG * delta * out[R.STRAIN_NORM][:, 0]
    rel = np.abs(nu_t - want).max() / np.abs(want).max()
    worst = float((np.abs(nu_t - want) / np.maximum(np.abs(want), 1e-300)).max() / eps)
    print(f"smagorinsky witness: max relative difference / eps = {worst:.3f} (bound 8), max-norm {rel / eps:.3f}")
    assert want.max() > 1e-4 and (np.abs(nu_t - want) <= 8.0 * eps * np.abs(want)).all()


# ------------------------------------------------------------------------------------------------ multi-block
@functools.lru_cache(maxsize=None)
def _mesh(name):
    """The mesh with fp32-exact vertex coordinates (what the fp32 library holds, and valid input of the fp64 one), random fp32-exact
    velocities and boundary values of two envs, and the restatement's ``(g, A)`` per env: computed once, shared by both dtypes."""
    spec = MESHES[name]()
    spec.blocks = [np.asarray(c, np.float64).astype(np.float32).astype(np.float64) for c in spec.blocks]
    dom = spec.oracle()
    rng = np.random.default_rng(11)
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    u = f32(0.5 * rng.standard_normal((2, dom.d, dom.N)))
    faces = [(b, f) for b, blk in enumerate(dom.blocks) for f in range(2 * dom.d) if dom.is_empty(b, f)]
    bvs = [{(b, f): f32(0.3 * rng.standard_normal(dom.blocks[b].bounds[f].velocity.shape)) for b, f in faces} for _ in range(2)]
    refs = []
    for e in range(2):
        R.set_oracle_boundary(dom, bvs[e])
        refs.append(R.multi_block_gradient(dom, u[e]))
    h_max = max(float(np.sqrt((np.linalg.inv(blk.Minv) ** 2).sum(axis=-2)).max()) for blk in dom.blocks)    # longest column of M
    u_max = max([np.abs(u).max()] + [np.abs(v).max() for bv in bvs for v in bv.values()])
    for g, _ in refs:
        R.assert_not_trivial(g, u_max, h_max)
    return spec, u, bvs, refs


def _native_mesh(spec, u, bvs, dtype):
    dom = spec.native(batch=len(bvs), dtype=dtype)
    dom.velocity.copy_(torch.as_tensor(u, dtype=dtype))
    for e, bv in enumerate(bvs):
        for (b, f), v in bv.items():
            dom.blocks[b].boundary(f)[e].copy_(torch.as_tensor(v, dtype=dtype))
    return dom


def _mb_state(dom):
    return [dom.velocity.clone(), dom.pressure.clone(), dom.boundary_velocity.clone()]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("name", list(MESHES))
def test_multi_block_kinds_against_the_restatement(name, dtype):
    spec, u, bvs, refs = _mesh(name)
    dom = _native_mesh(spec, u, bvs, dtype)
    dom.pressure.copy_(torch.randn(dom.pressure.shape, dtype=dtype, device=dom.device))
    before = _mb_state(dom)
    out = {kind: _np(dom.flow_diagnostic(kind)) for kind in R.KINDS}
    after = _mb_state(dom)
    n = dom.n_cells
    dom.close()
    assert all(torch.equal(a, b) for a, b in zip(before, after))
    for kind in R.KINDS:
        assert out[kind].shape == (2, R.channels(spec.dims, kind), n)
    _check_all_kinds(out, refs, spec.dims, _eps(dtype), f"mesh {name}")


# ------------------------------------------------------------------------------------------------ analytic: rigid rotation
def _check_rigid(out, A_per_env, dims, eps, what):
    for b, (omega, _) in enumerate(R.RIGID_2D if dims == 2 else R.RIGID_3D):
        A = A_per_env[b]
        w_exact, q_exact = R.rigid_expected(dims, omega)
        tol_w, tol_q, tol_s = R.rigid_bounds(A, eps)
        w = out[R.VORTICITY][b].reshape(tol_w.shape)
        err_w = np.abs(w - w_exact.reshape((-1,) + (1,) * (w.ndim - 1)))
        err_q = np.abs(out[R.Q][b].reshape(tol_q.shape) - q_exact)
        s = out[R.STRAIN_NORM][b].reshape(tol_s.shape)
        print(f"{what} env {b}: vorticity error / bound {float((err_w / tol_w).max()):.3f}, Q {float((err_q / tol_q).max()):.3f}, "
              f"strain norm / bound {float((s / tol_s).max()):.3f}")
        assert (err_w <= tol_w).all() and (err_q <= tol_q).all() and (s >= 0).all() and (s <= tol_s).all()      # wall cells included
        mag = out[R.VORTICITY_MAGNITUDE][b].reshape(tol_s.shape)
        assert (np.abs(mag - np.sqrt((w_exact ** 2).sum())) <= tol_w.sum(axis=0) + 8.0 * eps * mag).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("dims", [2, 3])
def test_rigid_rotation_on_a_uniform_single_block_grid(dims, dtype):
    case = R.rigid_single_case(dims)
    grid = case.grid()
    A = [R.single_block_gradient(case.oracle_domain(b, grid))[1] for b in range(case.B)]      # (the bound's scale only)
    ns = case.native(dtype=dtype)
    assert torch.equal(ns.velocity.cpu().double(), torch.as_tensor(case.velocity))            # the field is exact in this build
    out = {kind: _np(ns.flow_diagnostic(kind)) for kind in R.KINDS}
    ns.close()
    _check_rigid(out, A, dims, _eps(dtype), f"uniform {dims}-D")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_rigid_rotation_on_an_affine_two_block_mesh(dtype):
    spec, fields = R.rigid_affine_spec()
    oracle = spec.oracle()
    A = []
    for u, bv in fields:
        R.set_oracle_boundary(oracle, bv)
        A.append(R.multi_block_gradient(oracle, u)[1])
    dom = _native_mesh(spec, np.stack([u for u, _ in fields]), [bv for _, bv in fields], dtype)
    assert torch.equal(dom.velocity.cpu().double(), torch.as_tensor(np.stack([u for u, _ in fields])))
    out = {kind: _np(dom.flow_diagnostic(kind)) for kind in R.KINDS}
    dom.close()
    _check_rigid(out, A, 2, _eps(dtype), "affine two-block")


# ------------------------------------------------------------------------------------------------ untouched state
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_a_step_after_a_diagnostic_replays_bit_for_bit(dtype):
    case = make_case(dims=2, n=(32, 16), fixed_axes=(1,), B=2, seed=0, with_source=True, vel_scale=0.3)
    got = []
    for with_diagnostics in (False, True):
        ns = case.native(dtype=dtype)
        if with_diagnostics:
            for kind in R.KINDS:
                ns.flow_diagnostic(kind)
        ns.piso_step(0.03, advection_tol=1e-7, pressure_tol=1e-7)
        got.append((ns.velocity.clone(), ns.pressure.clone()))
        ns.close()
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])

    spec, u, bvs, _ = _mesh("split_rotated_channel")
    got = []
    for with_diagnostics in (False, True):
        dom = _native_mesh(spec, 0.4 * u, bvs, dtype)
        if with_diagnostics:
            for kind in R.KINDS:
                dom.flow_diagnostic(kind)
        dom.piso_step(0.02, advection_tol=1e-6, pressure_tol=1e-5, raise_on_failure=False)
        got.append((dom.velocity.clone(), dom.pressure.clone()))
        dom.close()
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])


# ------------------------------------------------------------------------------------------------ argument errors
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_argument_errors_raise_their_codes_and_leave_out_alone(dtype):
    from fluidgym_amd.native import NativeSolver

    ns = NativeSolver([np.full(8, 0.125, np.float32), np.full(6, 0.25, np.float32)], 2, fixed_faces=(2, 3), dtype=dtype, allocate=False)
    out = torch.full((2, 4, 6, 8), -7.0, dtype=dtype, device=ns.device)
    st = ctypes.c_void_p(torch.cuda.current_stream(ns.device).cuda_stream)
    po = ctypes.c_void_p(out.data_ptr())
    with pytest.raises(L.NativeLibraryError, match="status -2"):      # FG_ERR_NOT_BOUND: no velocity yet
        ns.flow_diagnostic(L.FG_DIAG_GRADIENT, out=out)
    ns.allocate_fields()
    assert ns.lib.fg_flow_diagnostic(ns.handle, 5, po, st) == L.FG_ERR_INVALID_ARG
    assert ns.lib.fg_flow_diagnostic(ns.handle, -1, po, st) == L.FG_ERR_INVALID_ARG
    assert ns.lib.fg_flow_diagnostic(ns.handle, L.FG_DIAG_Q, None, st) == L.FG_ERR_INVALID_ARG
    assert ns.lib.fg_flow_diagnostic(None, L.FG_DIAG_Q, po, st) == L.FG_ERR_INVALID_ARG
    with pytest.raises(ValueError):
        ns.flow_diagnostic(7)
    with pytest.raises(ValueError, match="out must be"):
        ns.flow_diagnostic(L.FG_DIAG_Q, out=out)                          # four channels offered, one needed
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    ns.flow_diagnostic(L.FG_DIAG_GRADIENT, out=out)                       # and the same tensor is written once the call is valid
    assert bool((out == 0.0).all())
    ns.close()

    spec, u, bvs, _ = _mesh("split_rotated_channel")
    dom = _native_mesh(spec, u, bvs, dtype)
    out = torch.full((2, 4, dom.n_cells), -7.0, dtype=dtype, device=dom.device)
    po = ctypes.c_void_p(out.data_ptr())
    assert dom.lib.fg_mb_flow_diagnostic(dom.handle, 5, po, st) == L.FG_ERR_INVALID_ARG
    assert dom.lib.fg_mb_flow_diagnostic(dom.handle, L.FG_DIAG_Q, None, st) == L.FG_ERR_INVALID_ARG
    assert dom.lib.fg_mb_flow_diagnostic(None, L.FG_DIAG_Q, po, st) == L.FG_ERR_INVALID_ARG
    with pytest.raises(ValueError, match="out must be"):
        dom.flow_diagnostic(L.FG_DIAG_VORTICITY, out=out)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    dom.close()


# ------------------------------------------------------------------------------------------------ env level
ENVS = {
    "RBC2D-easy-v0": dict(num_envs=2, n_heaters=4, resolution=8, step_length=0.1, load_initial_domain=False, load_domain_statistics=False),
    "TCFSmall3D-both-easy-v0": dict(num_envs=2, resolution_x_z=16, resolution_y=16, step_length=0.6, use_marl=False,
                                    randomize_initial_state=False),
    "CylinderJet2D-easy-v0": dict(num_envs=2, resolution=8, initial_domain_steps=6, randomize_initial_state=False, step_length=0.05,
                                  dt=0.01, episode_length=3),
}


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("env_id", list(ENVS))
def test_env_accessors(env_id, dtype):
    import fluidgym_amd

    env = fluidgym_amd.make(env_id, dtype=dtype, **ENVS[env_id])
    env.reset(seed=2)
    env.step(torch.zeros_like(env.sample_action()))
    vel = env.get_velocity()
    d = vel.shape[1]
    accessors = {L.FG_DIAG_GRADIENT: env.get_velocity_gradient, L.FG_DIAG_VORTICITY: env.get_vorticity,
                 L.FG_DIAG_VORTICITY_MAGNITUDE: env.get_vorticity_magnitude, L.FG_DIAG_Q: env.get_q_criterion,
                 L.FG_DIAG_STRAIN_NORM: env.get_strain_rate_norm}
    for kind, get in accessors.items():
        view, cells = get(), get(on_cells=True)
        assert view.shape == (vel.shape[0], L.diagnostic_channels(d, kind)) + vel.shape[2:]       # the grid of get_velocity()
        assert torch.equal(cells, env._domain.solver.flow_diagnostic(kind))                        # the domain-level call
        assert torch.equal(view, env._diagnostic_to_view(cells))                                   # the family's resampler, bit for bit
        if hasattr(env, "_resampler"):
            assert torch.equal(view, env._resampler(cells))
        else:
            assert torch.equal(view, cells)                                                        # plain single-block: the simulation grid
        assert bool(torch.isfinite(view).all()) and bool(torch.isfinite(cells).all())
    if env_id.startswith("Cylinder"):
        assert float(env.get_vorticity().abs().max()) > 0.0 and float(env.get_vorticity(on_cells=True).abs().max()) > 0.0
    env.close()
