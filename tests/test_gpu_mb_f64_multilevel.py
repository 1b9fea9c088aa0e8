"""The multilevel preconditioner in the fp64 build (``MultiBlockDomain(dtype=torch.float64).set_pressure_multilevel(fp64=True)``,
policy ``pressure_multilevel_fp64``): the apply kernels in doubles against the NumPy formula, the kernel-form preconditioned CG
(csrc/fg_mb_krylov.hip: k_ml_prolong_cg / k_mbc_ap<.., MBC_PRE> / k_mbc_update<.., true>) against its CPU replay, whole PISO steps against the
oracle's direct solves, off-means-off, replay, and the float64 envs under the policy."""
import ctypes

import numpy as np
import pytest
import torch

import helpers_mb as H
from test_gpu_mb_f64 import _rel, _state

pytestmark = pytest.mark.gpu


def _ml_reference(tab, P, r):
    """z = r / diag + (1 / 2s) Z4 D4^-1 Z4^T r + (1 / s) Z8 A8^+ Z8^T r with s = trace(P) / trace(S) (tests/test_gpu_mb.py)."""
    a4, p4 = tab["a4"], tab["parent4"]
    scale_inv = tab["geom_diag_sum"] / P.diagonal().sum()
    r4 = np.bincount(a4, weights=r, minlength=tab["n4"])
    r8 = np.bincount(p4, weights=r4, minlength=tab["n8"])
    return r / P.diagonal() + 0.5 * scale_inv * (r4 / tab["d4"])[a4] + scale_inv * (tab["aci8"] @ r8)[p4[a4]]


def _airfoil_domain(div, batch, dtype):
    from fluidgym_amd.envs.airfoil_grid import make_airfoil_mesh
    from fluidgym_amd.envs.cylinder_grid import build_domain

    return build_domain(make_airfoil_mesh(attack_angle_deg=10.0, resolution_div=div), 0.001, batch=batch, dtype=dtype)


_APPLY_CASES = [("polar_ring", 3), ("split_rotated_channel", 3), ("odd_channel", 3), ("airfoil4", 3), ("airfoil2", 3), ("polar_ring", 32),
                ("big_channel", 2)]


@pytest.mark.parametrize("mesh,B", _APPLY_CASES)
def test_multilevel_apply_in_doubles(mesh, B):
    """mb_ml_apply in the fp64 build against the NumPy formula on the same tables, within the 1e-12 the fp64 preconditioner forms
    are held to (tests/test_gpu_precond_forms.py); the same aggregate counts as the fp32 domain of the mesh.  In doubles k_ml_coarse
    has two reachable instances: four systems per workgroup (batch 3, and batch 32 as well -- the eight-systems form of the fp32
    build does not exist here, its partial sums alone are 64 KB of LDS) and two systems per workgroup on ``big_channel`` (the split
    channel at 400 x 256 cells: 1600 coarse aggregates, whose rows no longer fit 64 KB four systems at a time).  Batch 32 also
    covers a launch whose last workgroups hold fewer systems than their slots."""
    spec_of = lambda: H.split_rotated_channel(nx=400, ny=256, cut=200) if mesh == "big_channel" else getattr(H, mesh)()
    make = (lambda dt: _airfoil_domain(int(mesh[-1]), B if dt == torch.float64 else 1, dt)) if mesh.startswith("airfoil") else \
           (lambda dt: spec_of().native(batch=B if dt == torch.float64 else 1, dtype=dt))
    d32 = make(torch.float32)
    want = d32.set_pressure_multilevel()
    d32.close()
    dom = make(torch.float64)
    assert dom.set_pressure_multilevel() is None                 # still opt-in
    got = dom.set_pressure_multilevel(fp64=True)
    assert want is not None and got == want and set(got) == {"n4", "n8"}
    tab = dom._multilevel_tables
    P = dom.unit_pressure_matrix()           # leaves the A = 1 matrix assembled on the device
    N = dom.n_cells
    r = np.random.default_rng(3).standard_normal((B, N))
    z = dom.multilevel_apply(torch.from_numpy(r)).cpu().numpy()
    assert z.dtype == np.float64
    worst = max(_rel(z[b], _ml_reference(tab, P, r[b])) for b in range(B))
    print(f"MB_F64_ML_APPLY {mesh} x {B}: n4 {got['n4']} n8 {got['n8']} rel {worst:.2e}")
    assert worst < 1e-12, (mesh, B, worst)
    if mesh == "big_channel":
        assert got["n8"] > 1024
    dom.close()


def _load_buffer(dom, which, host):
    from fluidgym_amd import _lib as L

    hip = ctypes.CDLL("libamdhip64.so")
    ptr, cnt = ctypes.c_void_p(), ctypes.c_int64()
    L.check(dom.lib.fg_mb_get_buffer(dom.handle, which, ctypes.byref(ptr), ctypes.byref(cnt)), lib=dom.lib)
    t = torch.from_numpy(np.ascontiguousarray(host, np.float64)).to(dom.dtype).cuda()
    assert t.numel() == cnt.value
    assert hip.hipMemcpy(ptr, ctypes.c_void_p(t.data_ptr()), ctypes.c_size_t(t.element_size() * t.numel()), 3) == 0
    torch.cuda.synchronize()


def _pcg_restart(P, b, M, tol, maxit, perm=None, restart=100):
    """``tests/test_multilevel_precond.py::_pcg`` with the one rule of the kernels it leaves out -- the residual is recomputed and the
    direction reset every 100 iterations (mb_cg's CG_RESTART, the reference's residualResetSteps) -- and, for the spread of the
    iteration count, its dot products summed in a permuted order."""
    dot = (lambda u, v: float(np.sum((u * v)[perm]))) if perm is not None else (lambda u, v: float(u @ v))
    N = len(b)
    x = np.zeros(N); r = b.copy(); fresh = True
    for it in range(maxit):
        if it > 0 and it % restart == 0:
            r = b - P @ x; fresh = True
        rt = r - r.mean()
        if np.sqrt(dot(rt, rt) / N) < tol:
            return it
        z = M(rt) if M else rt.copy()
        z -= z.mean()
        rz = dot(rt, z)
        p = z if fresh else z + (rz / rz_prev) * p
        Ap = P @ p
        alpha = rz / dot(p, Ap)
        x += alpha * p; r -= alpha * Ap
        rz_prev = rz; fresh = False
    return maxit


def _cylinder_system(dom, spec):
    """Matrix (A = 100 (1 + 0.3 u)) and right-hand side of test_multilevel_precond.py on the cylinder mesh, as CSR + the [F][N] arrays."""
    from test_mb_tables import HostTables
    from test_multilevel_precond import _pressure_matrix

    N, F = dom.n_cells, 4
    t = HostTables(spec)
    A = 100.0 * (1.0 + 0.3 * np.random.default_rng(0).random(N))
    P = _pressure_matrix(t, 1.0 / A)
    t.close()
    nbr = dom.neighbors()
    off = np.zeros((F, N))
    for f in range(F):
        ok = nbr[f] >= 0
        off[f][ok] = np.asarray(P[np.nonzero(ok)[0], nbr[f][ok]]).ravel()
    cc = np.concatenate([0.25 * (c[:, :-1, :-1] + c[:, 1:, :-1] + c[:, :-1, 1:] + c[:, 1:, 1:]).reshape(2, -1) for c in spec.blocks], 1)
    xs = np.sin(0.7 * cc[0]) * np.cos(1.3 * cc[1]) + 0.3 * np.sin(2.1 * cc[0] + cc[1])
    b = P @ xs
    b -= b.mean(); b /= np.sqrt(b @ b / N)
    return P, P.diagonal(), off, b


def test_preconditioned_cg_iteration_counts_against_the_cpu_replay():
    """One fp64 mb_cg solve on the reference's cylinder mesh (resolution 24, 14 232 cells) with the matrix and right-hand side of
    test_multilevel_precond.py (A = 100 (1 + 0.3 u)), loaded through the domain's buffers, with and without the preconditioner.

    The reference is the CPU replay of the kernels' recurrence, ``test_multilevel_precond.py::_pcg``.  It restates the recurrence
    WITHOUT the restart every 100 iterations (residual recomputed from the iterate, direction reset) that mb_cg and the reference's
    CG have, and on this non-symmetric matrix the recurrence residual of a CG that never restarts stops falling: at RMS 1e-10
    ``_pcg`` ends at a cap of 5000 in both forms and never gets below 1.5e-4 (plain) / 1.3e-6 (preconditioned) in 3000 iterations.
    1e-3 is the smallest decade its plain form reaches, so both counts are compared at 1e-3: ``_pcg`` 357 plain / 95 preconditioned.
    The plain solve passes three restarts on the way, so the GPU's plain count is held to ``_pcg_restart`` above (``_pcg`` plus that
    one rule: 397 / 95), the preconditioned one (no restart before 95) to ``_pcg`` itself as well.  Spread of the counts over three
    permuted summation orders of the dot products: 0 / 0, so the GPU may differ by one.  Measured on the GPU (MI355X, fp64 build):
    397 / 95.
    With the restart the replay has no floor (7.5e-8 plain, 1.8e-18 preconditioned after 3000 iterations), so the preconditioned
    count is compared once more where the recurrence in doubles matters, at 1e-10 (cap 20 000, the cap of the fp64 oracle tests):
    ``_pcg_restart`` 266 in all three orders, GPU 265.  The plain solve needs ~4000 iterations and 39 restarts there, and its count
    moves by tens with the summation order -- CPU 3972 ... 3998 over seven orders, GPU 3946 -- so it is printed and held to
    convergence and to "more than the preconditioned one", not to a count."""
    from fluidgym_amd import _lib as L
    from test_multilevel_precond import _cylinder_spec, _pcg

    CAP = 20000
    spec = _cylinder_spec(24)
    dom = spec.native(batch=1, dtype=torch.float64)
    N = dom.n_cells
    assert dom.set_pressure_multilevel(fp64=True) is not None
    dom.set_stall_limit(CAP)          # the replay has no stall rule: the solves end on the tolerance or the cap
    tab = dom._multilevel_tables
    P, diag, off, b = _cylinder_system(dom, spec)
    _load_buffer(dom, L.FG_MB_BUF_P_DIAG, diag[None])
    _load_buffer(dom, L.FG_MB_BUF_P_OFF, off[None])
    _load_buffer(dom, L.FG_MB_BUF_DIV, b[None])
    M = lambda r: _ml_reference(tab, P, r)
    perms = [np.random.default_rng(s).permutation(N) for s in (1, 2, 3)]
    for TOL in (1e-3, 1e-10):
        # CPU: the replay, and the spread of its count over three summation orders
        ref = {"plain": _pcg_restart(P, b, None, TOL, CAP), "pre": _pcg_restart(P, b, M, TOL, CAP)}
        counts = {"plain": [_pcg_restart(P, b, None, TOL, CAP, pm) for pm in perms], "pre": [_pcg_restart(P, b, M, TOL, CAP, pm) for pm in perms]}
        spread = {k: max(v + [ref[k]]) - min(v + [ref[k]]) for k, v in counts.items()}
        assert ref["plain"] < CAP and ref["pre"] < CAP
        # GPU
        assert dom.set_pressure_multilevel(fp64=True) is not None      # (re-installs the tables: leaves the A = 1 matrix in the buffers)
        _load_buffer(dom, L.FG_MB_BUF_P_DIAG, diag[None])
        _load_buffer(dom, L.FG_MB_BUF_P_OFF, off[None])
        before = dom.config_dump()["multilevel_cg_solves"]
        pre = dom.debug_pressure_cg(TOL, CAP, project_mean=True)
        assert dom.config_dump()["multilevel_cg_solves"] == before + 1
        dom.set_pressure_multilevel(False, fp64=True)
        plain = dom.debug_pressure_cg(TOL, CAP, project_mean=True)
        assert dom.config_dump()["multilevel_cg_solves"] == before + 1
        print(f"MB_F64_ML_PCG tol {TOL:g}: GPU plain {plain['iterations'][0]} pre {pre['iterations'][0]} | CPU replay plain {ref['plain']} pre {ref['pre']} "
              f"permuted {counts} spread {spread} | residuals {plain['residual'][0]:.3e} {pre['residual'][0]:.3e}")
        assert pre["converged"][0] and plain["converged"][0]
        assert pre["iterations"][0] < plain["iterations"][0]
        assert abs(pre["iterations"][0] - ref["pre"]) <= spread["pre"] + 1, (TOL, pre, ref, spread)
        if TOL == 1e-3:
            assert abs(plain["iterations"][0] - ref["plain"]) <= spread["plain"] + 1, (TOL, plain, ref, spread)
            pcg_pre = _pcg(P, b, M, TOL, CAP)
            assert pcg_pre < 100 and abs(pre["iterations"][0] - pcg_pre) <= spread["pre"] + 1, (pre, pcg_pre, spread)
    dom.close()


def test_fp32_library_reaches_the_same_loop_through_its_debug_switch(monkeypatch):
    """FG_MB_PCG_KERNEL=1 (read at fg_mb_create, off by default): the fp32 library runs the preconditioned pressure CG as the
    kernel-form loop -- the fp32 instances of k_ml_prolong_cg / k_mbc_ap<.., MBC_PRE> / k_mbc_update<.., true> -- instead of its on-chip / cluster
    kernels.  Same system, tolerance 1e-3 (the fp32 recurrence residual of this matrix, entries ~1e-2 .. 1, is good to ~1e-6), from the
    loaded buffers: the count against the CPU replay and against the fp64 build's 95.  Another summation order and fp32 rounding of
    the dot products move a CG count by one or two (the bound tests/test_gpu_mb.py holds its kernel forms to among each other).
    And a whole PISO step under the switch against the oracle at the bounds of the fp32 preconditioned step
    (test_gpu_mb.py::test_multilevel_preconditioned_step_matches_the_oracle), in as many pressure iterations (+- 2) as the on-chip kernel."""
    from fluidgym_amd import _lib as L
    from test_multilevel_precond import _cylinder_spec

    def step(spec, d):
        dom = spec.native(batch=2)
        assert dom.set_pressure_multilevel() is not None
        states = [_state(d, 10 + b) for b in range(2)]
        for b, (u, p) in enumerate(states):
            dom.velocity[b] = torch.as_tensor(u, dtype=torch.float32)
            dom.pressure[b] = torch.as_tensor(p, dtype=torch.float32)
        its = dom.piso_step([0.05, 0.03], advection_tol=1e-7, pressure_tol=2e-6, pressure_use_bicgstab=False, pressure_project_mean=True)
        out = (its, dom.velocity.cpu().numpy().astype(np.float64), dom.pressure.cpu().numpy().astype(np.float64), dom.config_dump(), states)
        dom.close()
        return out

    spec = H.polar_ring()
    d = spec.oracle()
    its_oc, _, _, cfg_oc, _ = step(spec, d)
    assert cfg_oc["FG_MB_PCG_KERNEL"] == 0 and cfg_oc["multilevel_cg_solves"] == 0
    monkeypatch.setenv("FG_MB_PCG_KERNEL", "1")
    its_k, u, p, cfg_k, states = step(spec, d)
    assert cfg_k["FG_MB_PCG_KERNEL"] == 1 and cfg_k["multilevel_cg_solves"] == 2
    print(f"MB_F32_PCG_KERNEL polar_ring: iterations kernel form {its_k} on-chip {its_oc}")
    assert abs(its_k[1] - its_oc[1]) <= 2 and abs(its_k[2] - its_oc[2]) <= 2
    for b, dt in enumerate([0.05, 0.03]):
        u_ref, p_ref = d.piso_step(states[b][0], states[b][1], dt)
        eu, ep = _rel(u[b], u_ref), _rel(p[b] - p[b].mean(), p_ref - p_ref.mean())
        print(f"MB_F32_PCG_KERNEL polar_ring env {b}: velocity {eu:.2e} pressure {ep:.2e}")
        assert eu < 2e-4 and ep < 2e-3
    # the cylinder system of the test above, in fp32
    cspec = _cylinder_spec(24)
    dom = cspec.native(batch=1)
    assert dom.set_pressure_multilevel() is not None
    tab = dom._multilevel_tables
    P, diag, off, bvec = _cylinder_system(dom, cspec)
    _load_buffer(dom, L.FG_MB_BUF_P_DIAG, diag[None])
    _load_buffer(dom, L.FG_MB_BUF_P_OFF, off[None])
    _load_buffer(dom, L.FG_MB_BUF_DIV, bvec[None])
    ref = _pcg_restart(P, bvec, lambda r: _ml_reference(tab, P, r), 1e-3, 5000)
    got = dom.debug_pressure_cg(1e-3, 5000, project_mean=True)
    print(f"MB_F32_PCG_KERNEL cylinder mesh tol 1e-3: GPU fp32 kernel form {got['iterations'][0]} CPU replay {ref} residual {got['residual'][0]:.3e}")
    assert dom.config_dump()["multilevel_cg_solves"] == 1
    assert got["converged"][0] and abs(got["iterations"][0] - ref) <= 2
    dom.close()


def _oracle_step(spec_fn, bicg, multilevel):
    """The case of test_gpu_mb_f64.py::test_fp64_piso_step_matches_the_oracle, with or without the preconditioner installed."""
    from fluidgym_amd import _lib as L

    spec = spec_fn()
    d = spec.oracle()
    B = 2
    dom = spec.native(batch=B, dtype=torch.float64)
    if multilevel:
        assert dom.set_pressure_multilevel(fp64=True) is not None
    dt = [0.05, 0.03]
    states = [_state(d, 10 + b) for b in range(B)]
    for b, (u, p) in enumerate(states):
        dom.velocity[b] = torch.as_tensor(u, dtype=torch.float64)
        dom.pressure[b] = torch.as_tensor(p, dtype=torch.float64)
    dom.solver_counters(reset=True)
    its = dom.piso_step(dt, advection_tol=1e-13, pressure_tol=1e-13, pressure_use_bicgstab=bicg, max_iterations=20000, raise_on_failure=False,
                        pressure_project_mean=not bicg)
    assert its[0] > 0 and its[1] > 0
    u_gpu, p_gpu = dom.velocity.cpu().numpy(), dom.pressure.cpu().numpy()
    nd = d.d
    A = dom.buffer(L.FG_MB_BUF_A).view(B, -1).cpu().numpy()
    Coff = dom.buffer(L.FG_MB_BUF_C_OFF).view(B, 2 * nd, -1).cpu().numpy()
    rhs = dom.buffer(L.FG_MB_BUF_RHS).view(B, nd, -1).cpu().numpy()
    Pd = dom.buffer(L.FG_MB_BUF_P_DIAG).view(B, -1).cpu().numpy()
    Po = dom.buffer(L.FG_MB_BUF_P_OFF).view(B, 2 * nd, -1).cpu().numpy()
    out = []
    for b in range(B):
        trace = {}
        u_ref, p_ref = d.piso_step(states[b][0], states[b][1], dt[b], trace=trace)
        out.append({"A": _rel(A[b], trace["C"][0]), "Coff": _rel(Coff[b], trace["C"][1]), "rhs": _rel(rhs[b], trace["rhs"]),
                    "Pdiag": _rel(Pd[b], trace["P"][0]), "Poff": _rel(Po[b], trace["P"][1]),
                    "velocity": _rel(u_gpu[b], u_ref), "pressure": _rel(p_gpu[b] - p_gpu[b].mean(), p_ref - p_ref.mean())})
    res = (out, its, dom.solver_counters(), dom.multilevel_status(), dom.config_dump()["multilevel_cg_solves"], dom.env_status())
    dom.close()
    return res


@pytest.mark.parametrize("spec_fn", [H.split_rotated_channel, H.polar_ring, H.odd_channel, H.skewed_pair, H.twisted_ring])
@pytest.mark.parametrize("bicg", [0, 1])
def test_fp64_preconditioned_piso_step_matches_the_oracle(spec_fn, bicg):
    """Whole PISO steps against the oracle's direct solves with the preconditioner installed, on the five 2-D meshes of
    test_gpu_mb_f64.py::test_fp64_piso_step_matches_the_oracle -- once through the preconditioned CG (pressure_project_mean), once
    through the pressure BiCGStab's trial with the unfused apply -- at its arguments and bounds (tolerances 1e-13, cap 20 000;
    assembly < 1e-11, velocity < 1e-8, pressure < 1e-7): the converged answer is the same system's.  The preconditioned path must
    actually have run, in fewer pressure iterations than the plain run on the same state (same arguments: the CG runs project
    the mean, the BiCGStab runs do not).  skewed_pair and twisted_ring are the non-orthogonal meshes (the plain fp64 test solves
    them with BiCGStab): a trial attempt may fail there and be repeated plain (measured: one of the two on twisted_ring), so for
    BiCGStab the status is held to "attempts were made", not to "none failed".
    CG is no solver for the non-symmetric pressure matrices of those two meshes, with or without the preconditioner: the plain
    fp64 CG ends both correctors unconverged on a best iterate that is 0.5 - 1.0 (relative) from the oracle (414 / 234 and
    1321 / 1116 iterations, env status 1), the preconditioned recurrence breaks down in the first corrector (309 and 643
    iterations, non-finite after its recoveries) and the envs' steps are not committed (env status 2).  That is asserted as
    such -- the runs end, the failure is reported, nothing is claimed about the answer -- instead of the bounds."""
    errs, its, ctr, status, cg_solves, env_status = _oracle_step(spec_fn, bicg, True)
    errs0, its0, ctr0, status0, cg_solves0, env_status0 = _oracle_step(spec_fn, bicg, False)
    for b, e in enumerate(errs):
        print(f"MB_F64_ML_ERR {spec_fn.__name__} bicg {bicg} env {b}: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    print(f"MB_F64_ML_ITS {spec_fn.__name__} bicg {bicg}: preconditioned {its} plain {its0} status {status} cg solves {cg_solves} "
          f"unconverged {ctr['pressure0']['unconverged']} {ctr['pressure1']['unconverged']} (plain {ctr0['pressure0']['unconverged']} {ctr0['pressure1']['unconverged']}) "
          f"env status {env_status.tolist()} (plain {env_status0.tolist()}); plain velocity / pressure error {max(e['velocity'] for e in errs0):.2e} / {max(e['pressure'] for e in errs0):.2e}")
    if not bicg and spec_fn in (H.skewed_pair, H.twisted_ring):
        for e in errs:
            for k in ("A", "Coff", "rhs", "Pdiag", "Poff"):
                assert e[k] < 1e-11, (k, e)
        assert cg_solves >= 1 and cg_solves0 == 0
        assert ctr0["pressure0"]["unconverged"] == 2 and ctr0["pressure1"]["unconverged"] == 2 and (env_status0 != 0).all()     # plain CG: no solver here
        assert ctr["pressure0"]["unconverged"] > 0 and (env_status != 0).all()                                                    # reported, not hidden
        return
    for e in errs:
        for k in ("A", "Coff", "rhs", "Pdiag", "Poff"):
            assert e[k] < 1e-11, (k, e)
        assert e["velocity"] < 1e-8 and e["pressure"] < 1e-7, e
    if bicg:
        assert status["attempts"] > 0 and status0["attempts"] == 0, (status, status0)
        assert cg_solves == 0
    else:
        assert cg_solves == 2 and cg_solves0 == 0 and status["attempts"] == 0     # one solve per corrector, none by the plain loop
    assert ctr["pressure0"]["unconverged"] == 0 and ctr["pressure1"]["unconverged"] == 0
    assert its[1] < its0[1] and its[2] < its0[2], (its, its0)
    assert ctr["pressure0"]["mean"] < ctr0["pressure0"]["mean"] and ctr["pressure1"]["mean"] < ctr0["pressure1"]["mean"]


def _two_steps(dom, d):
    for b in range(dom.batch):
        u, p = _state(d, 30 + b)
        dom.velocity[b] = torch.as_tensor(u, dtype=torch.float64)
        dom.pressure[b] = torch.as_tensor(p, dtype=torch.float64)
    for _ in range(2):
        dom.piso_step([0.05, 0.03], advection_tol=1e-10, pressure_tol=1e-10, max_iterations=20000, pressure_project_mean=True)
    return dom.velocity.clone(), dom.pressure.clone()


def test_off_means_off():
    """A float64 domain that never asked, and one that installed the tables and switched them off again, compute the same bits;
    the policy that would ask is off by default."""
    from fluidgym_amd.simulation.policy import get_solver_policy

    assert get_solver_policy()["pressure_multilevel_fp64"] is False
    spec = H.polar_ring()
    d = spec.oracle()
    a = spec.native(batch=2, dtype=torch.float64)
    ua, pa = _two_steps(a, d)
    assert a.config_dump()["multilevel_cg_solves"] == 0
    a.close()
    b = spec.native(batch=2, dtype=torch.float64)
    assert b.set_pressure_multilevel(fp64=True) is not None
    assert b.set_pressure_multilevel(enable=False, fp64=True) is None
    ub, pb = _two_steps(b, d)
    assert b.config_dump()["multilevel_cg_solves"] == 0 and b.config_dump()["multilevel_on"] == 0
    assert torch.equal(ua, ub) and torch.equal(pa, pb)
    # and switched on, the same domain takes the preconditioned loop (so the comparison above compared something)
    assert b.set_pressure_multilevel(fp64=True) is not None
    _two_steps(b, d)
    assert b.config_dump()["multilevel_cg_solves"] == 4
    b.close()


def test_policy_on_replays_bit_for_bit():
    """``get_state -> set_state -> step`` on a float64 cylinder env under the policy is bit-identical, and the two identical envs of
    the batch stay identical (every sum of the preconditioned loop is a fixed-order tree into the order-independent accumulators)."""
    import fluidgym_amd

    old = fluidgym_amd.set_solver_policy(pressure_multilevel_fp64=True)
    try:
        env = fluidgym_amd.make("CylinderJet2D-easy-v0", num_envs=2, dtype=torch.float64, initial_domain_steps=2, randomize_initial_state=False)
        env.reset(seed=1)
        assert env._multilevel is not None and set(env._multilevel) == {"n4", "n8"}
        a = torch.tensor([[0.5], [0.5]], device="cuda", dtype=torch.float64)
        env.step(a)
        s0 = env.get_state()
        r1 = env.step(a)
        u1, p1 = env._domain.velocity.clone(), env._domain.pressure.clone()
        env.set_state(s0)
        r2 = env.step(a)
        assert env._domain.config_dump()["multilevel_cg_solves"] > 0
        assert torch.equal(u1, env._domain.velocity) and torch.equal(p1, env._domain.pressure)
        assert torch.equal(r1[1], r2[1]) and torch.equal(r1[0]["velocity"], r2[0]["velocity"])
        assert torch.equal(u1[0], u1[1]) and torch.equal(p1[0], p1[1])
        env.close()
    finally:
        fluidgym_amd.set_solver_policy(pressure_multilevel_fp64=old["pressure_multilevel_fp64"])


@pytest.mark.parametrize("env_id", ["CylinderJet2D-easy-v0", "Airfoil2D-easy-v0"])
def test_fp64_envs_step_under_the_policy(env_id):
    """The float64 envs of the two multi-block families with policy ``pressure_multilevel_fp64``: outputs float64 and finite, fewer
    pressure iterations over two env steps than with the policy off, and the fp32-against-fp64 gaps inside the bounds
    test_gpu_mb_f64.py::test_fp64_multi_block_envs_step uses (printed; DESIGN.md 4b records them)."""
    import fluidgym_amd

    def run(dtype, policy):
        old = fluidgym_amd.set_solver_policy(pressure_multilevel_fp64=policy)
        try:
            env = fluidgym_amd.make(env_id, num_envs=2, dtype=dtype, initial_domain_steps=3, randomize_initial_state=False)
            obs, _ = env.reset(seed=0)
            act = torch.full_like(env._zero_action, 0.25)
            env._domain.solver_counters(reset=True)
            for _ in range(2):
                obs, rew, term, trunc, info = env.step(act)
            assert all(v.dtype == dtype for v in obs.values()) and rew.dtype == dtype
            assert all(torch.isfinite(v).all() for v in obs.values()) and torch.isfinite(rew).all()
            ctr, status, ml = env._domain.solver_counters(), env._domain.multilevel_status(), env._multilevel
            out = (obs["velocity"].double().cpu().numpy(), info["drag"].double().cpu().numpy(), ctr, status, ml)
            env.close()
            return out
        finally:
            fluidgym_amd.set_solver_policy(pressure_multilevel_fp64=old["pressure_multilevel_fp64"])

    f32 = run(torch.float32, False)
    off = run(torch.float64, False)
    on = run(torch.float64, True)
    assert off[4] is None and on[4] is not None and on[4] == f32[4]
    gap = lambda x: (np.abs(f32[0] - x[0]).max() / np.abs(x[0]).max(), np.abs(f32[1] - x[1]).max() / np.abs(x[1]).max())
    (dv0, dd0), (dv1, dd1) = gap(off), gap(on)
    its = lambda x: (x[2]["pressure0"]["mean"], x[2]["pressure1"]["mean"])
    print(f"MB_F64_ML_ENV {env_id}: fp32 against fp64, velocity obs / drag: policy off {dv0:.2e} / {dd0:.2e}, policy on {dv1:.2e} / {dd1:.2e}; "
          f"pressure iterations per solve (corrector 0, 1): off {its(off)} on {its(on)} fp32 {its(f32)}; trial status {on[3]}")
    assert its(on)[0] < its(off)[0] and its(on)[1] < its(off)[1]
    assert dv1 < 5e-2 and dd1 < (0.3 if env_id.startswith("Airfoil") else 5e-2)
