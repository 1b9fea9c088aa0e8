"""Every form of the multi-block pressure CG held to the fp64 residual of the x it hands back (FG_MB_BUF_PRESSURE_X), not to the
residual it reports: the recurrence residual r is updated independently of x, so a solve can report 1e-6 and return something else.
The quantities and the bound are those of tests/mb_cg_ref.py (derived there; its teeth are shown on the CPU by
tests/test_mb_cg_ref_host.py):

    |true - reported| <= 4 max(g_ref, U)       and, where the solve reports convergence,       true <= tol + 4 max(g_ref, U)

Part A -- the chunked kernels (``fg_mb_krylov.hip::mb_cg``) on the systems, cases, switches and caps of tests/test_gpu_mbc_forms.py:
the caps 20 and 40 end unconverged (the iterate handed back is the kept one and carries the residual reported), 120 crosses a
restart, 5000 converges; the fp64 cases (tolerance 1e-12) are the sharp ones where they converge -- at the short caps the residual
word of the ABI is a float, whose rounding (2^-24 of a residual of 0.2) the reference reports through as well, so it sits in g_ref.
What the caps can see: a restart rebuilds r = b - P x from x, after which the reported residual carries a defect of x itself and the
solve repairs it (tests/test_mb_cg_ref_host.py), so a wrong x update shows in the gap only if it is made behind the last restart --
every update at the caps 20 and 40, the last 20 of cap 120, the iterations since the last multiple of 100 of a converged solve.
The same holds for the several hundred iterations of the unpreconditioned cases of part B.
For the preconditioned forms (``polar_ring`` here, every multilevel case of part B) g_ref and max_k|x_k| come from ANOTHER trajectory:
the reference restates the plain recurrence, as the issue behind this file specifies, and needs more iterations with larger
intermediate residuals than the kernels' preconditioned one -- the bound is one to two orders above the gaps measured there.
Part B -- the whole-solve forms (``k_mbc_onchip`` with 4 / 8 / 16 cells per thread, its aggregate-owned layout, ``k_mbc_l2``,
``k_mbc_cluster``) on the reference's cylinder mesh at the resolutions that select them, under the switch sets the existing tests
launch there (tests/test_gpu_mb.py, tests/test_gpu_cluster.py, tests/test_gpu_mb_driver_forms.py): the x of the last solve of a PISO
step against the matrix and right-hand side of that solve.  The step's mean removal runs over the iterate in place, so after a step
the buffer must equal ``Domain.pressure`` bit for bit.  A PISO step reports no residual per env, so the same system is then solved
once more from zero by ``debug_pressure_cg`` (same handle, same form -- the cluster counter is read around it), which does: that
solve is held to both bounds, and its untouched x to ``Domain.pressure`` = x - mean(x).
Part C -- one cell per thread on a 3-D mesh (``helpers_mb.odd_channel_3d``) in both libraries, the fp64 one also against the oracle.

Worst ratios |true - reported| / max(g_ref, U) measured: DESIGN.md, section 3."""
import numpy as np
import pytest
import torch

from tests import helpers_mb as H
from tests import mb_cg_ref as R
from tests.test_gpu_mbc_forms import B, CAPS, CASES, GOLDEN, SWITCHES, case_key, open_case

pytestmark = pytest.mark.gpu

# every switch that selects a form of the pressure CG: a case sets its own and clears the rest (read at fg_mb_create)
FORM_SWITCHES = ("FG_MB_ONCHIP", "FG_MB_CLUSTER", "FG_MB_PCG_KERNEL", "FG_MB_OC_AGG", "FG_MB_OC_RTG_NT", "FG_MB_OC_VARIANT", "FG_MB_CL_HALF",
                 "FG_MB_CL_MAXCL", "FG_MB_CL_NEAR")


def _switches(monkeypatch, env):
    for k in FORM_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _buf(dom, which, *shape):
    return dom.buffer(which).view(dom.batch, *shape).cpu().numpy()


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("lib,mesh,pre,pm", CASES)
def test_chunked_cg_iterate_leaves_the_residual_it_reports(lib, mesh, pre, pm, golden, monkeypatch):
    from fluidgym_amd import _lib as L

    _switches(monkeypatch, SWITCHES)
    diag, off, rhs, yp = golden[mesh + ".diag"], golden[mesh + ".off"], golden[mesh + ".rhs"], golden[mesh + ".yp"]
    tol = float(golden["tol." + lib])
    dom = open_case(lib, mesh, pre, pm, diag, off, rhs, yp)
    nbr, N, dtype = dom.neighbors(), dom.n_cells, dom._np
    worst = 0.0
    for cap in CAPS:
        info = dom.debug_pressure_cg(tol, cap, project_mean=(pm != 0))
        x = _buf(dom, L.FG_MB_BUF_PRESSURE_X, N)
        assert x.dtype == dtype
        for b in range(B):
            g_ref, U = R.gap_terms(diag[b], off[b], nbr, rhs[b], yp, pm, tol, cap, dtype)
            label = f"{case_key(lib, mesh, pre, pm)}.cap{cap} env {b} (iterations {info['iterations'][b]}, converged {int(info['converged'][b])})"
            worst = max(worst, R.check_solution(label, diag[b], off[b], nbr, rhs[b], x[b], info["residual"][b], info["converged"][b],
                                                yp, pm, tol, g_ref, U, dtype))
    print(f"MB_CG_WORST_RATIO {case_key(lib, mesh, pre, pm)}: {worst:.3f}")
    dom.close()


def _held_step(label, dom, dt, tol, stall_limit, step_kw, cap=5000, cluster=False):
    """One PISO step of ``dom``, then the assertions of parts B and C on its last pressure solve and on a solve of the same system by
    ``debug_pressure_cg`` (which must be a cluster solve where ``cluster``, and none otherwise).  Returns the worst gap ratio of the latter."""
    from fluidgym_amd import _lib as L

    N, F, dtype = dom.n_cells, 2 * dom.dims, dom._np
    eps = float(np.finfo(dtype).eps)
    nbr = dom.neighbors()
    dom.solver_counters(reset=True)
    dom.piso_step(dt, pressure_tol=tol, pressure_project_mean=True, max_iterations=cap, **step_kw)
    diag, off, rhs = _buf(dom, L.FG_MB_BUF_P_DIAG, N), _buf(dom, L.FG_MB_BUF_P_OFF, F, N), _buf(dom, L.FG_MB_BUF_DIV, N)
    x = _buf(dom, L.FG_MB_BUF_PRESSURE_X, N)
    pressure = dom.pressure.cpu().numpy()
    ctr = dom.solver_counters()
    assert ctr["pressure0"]["unconverged"] == 0 and ctr["pressure1"]["unconverged"] == 0 and ctr["pressure1"]["systems"] == dom.batch, ctr
    assert ctr["pressure1"]["max"] > 0, ctr      # the solve did iterate
    terms = [R.gap_terms(diag[b], off[b], nbr, rhs[b], None, 1, tol, cap, dtype, stall_limit) for b in range(dom.batch)]
    for b, (g_ref, U) in enumerate(terms):
        true = R.true_residual(diag[b], off[b], nbr, rhs[b], x[b], None, 1, dtype)
        print(f"MB_CG_TRUE_RES {label}.step env {b}: reported (below tol {tol:.1e}) true {true:.6e} g_ref {g_ref:.3e} U {U:.3e}")
        assert np.isfinite(x[b]).all()
        assert true <= tol + R.GAP_FACTOR * max(g_ref, U), (label, b, true, tol, g_ref, U)
        # the step's mean removal (k_mb_sub_mean) writes one value to the iterate, in place, and to the bound pressure: after a step
        # the buffer IS Domain.pressure, bit for bit (a copy from another env or through a wrong map shows here)
        assert np.array_equal(pressure[b], x[b]), (label, b, np.abs(pressure[b] - x[b]).max())
    solves = dom.config_dump()["cluster_solves"]
    info = dom.debug_pressure_cg(tol, cap, project_mean=True)
    assert (dom.config_dump()["cluster_solves"] - solves == 1) == cluster, (label, "the solve held to the gap bound ran in another form")
    x = _buf(dom, L.FG_MB_BUF_PRESSURE_X, N)
    worst = 0.0
    u = 0.5 * eps
    depth = -(-N // 2048) - 1 + 8 + 3 + 1 + 1
    for b, (g_ref, U) in enumerate(terms):
        assert info["converged"][b], (label, info)
        # this solve repeats the step's last one (same system, from zero, same form: the sums are order-fixed), so x is the iterate
        # the step's mean removal saw, and pressure = fl(x - m) with m the mean the kernels formed.  Every x_i - pressure_i is m to
        # one rounding of the subtraction, u |pressure_i|; so is their fp64 mean m_hat, hence 2 u max|pressure| between them
        c = x[b].astype(np.float64) - pressure[b].astype(np.float64)
        m_hat = c.mean()
        assert np.abs(c - m_hat).max() <= 2 * u * np.abs(pressure[b]).max(), (label, b, np.abs(c - m_hat).max(), u * np.abs(pressure[b]).max())
        # and m is the mean of x: k_mb_sum adds ceil(N / 2048) terms per thread in turn, eight levels in the workgroup, three over
        # the eight partials, k_mb_sub_mean divides -- `depth` roundings (one spare for the second order), each of at most u times
        # the sum of |x| so far, over N; plus the rounding that m_hat itself carries (above)
        x64 = x[b].astype(np.float64)
        slack = depth * u * np.abs(x64).mean() + u * np.abs(pressure[b]).max()
        assert abs(m_hat - x64.mean()) <= slack, (label, b, abs(m_hat - x64.mean()), slack)
        worst = max(worst, R.check_solution(f"{label}.solve env {b} (iterations {info['iterations'][b]})", diag[b], off[b], nbr, rhs[b], x[b],
                                            info["residual"][b], True, None, 1, tol, g_ref, U, dtype))
    print(f"MB_CG_WORST_RATIO {label}: {worst:.3f}")
    return worst


# (name, resolution of the cylinder mesh, switches, multilevel preconditioner + stall limit 5000, tolerance, cluster solves expected)
# plain recurrence at 1e-6 as test_onchip_cg_matches_the_chunked_cg; preconditioned at 1e-7 with the stall limit of
# test_aggregate_owned_onchip_cg_is_the_cell_ordered_one / test_l2_form_onchip_cg_is_the_register_resident_one / test_gpu_cluster.py.
# The preconditioned one-workgroup forms need FG_MB_CLUSTER=0 above 8 k cells (tests/test_gpu_mb_driver_forms.py: cluster0.agg1 /
# cluster0.agg0; tests/test_gpu_cluster.py: mode "0").  FG_MB_OC_RTG_NT=1 is launched today with the cluster left on, which then takes
# the solve: the case runs that switch set as it stands and records which form solved
WHOLE_SOLVE_CASES = [
    ("onchip4.r8", 8, {}, False, 1e-6, False),
    ("onchip8.r16", 16, {}, False, 1e-6, False),
    ("onchip16.r24", 24, {"FG_MB_ONCHIP": "1"}, False, 1e-6, False),
    ("onchip16.agg.r24", 24, {"FG_MB_CLUSTER": "0", "FG_MB_OC_AGG": "1"}, True, 1e-7, False),
    ("onchip16.cell.r24", 24, {"FG_MB_CLUSTER": "0", "FG_MB_OC_AGG": "0"}, True, 1e-7, False),
    ("cluster.r24", 24, {"FG_MB_CLUSTER": "1"}, True, 1e-7, True),
    ("l2.r32", 32, {"FG_MB_CLUSTER": "0"}, True, 1e-7, False),
    ("rtg_nt1.r32", 32, {"FG_MB_OC_RTG_NT": "1"}, True, 1e-7, True),
    ("cluster.half1.r32", 32, {"FG_MB_CLUSTER": "1", "FG_MB_CL_HALF": "1"}, True, 1e-7, True),
    ("cluster.half0.r32", 32, {"FG_MB_CLUSTER": "1", "FG_MB_CL_HALF": "0"}, True, 1e-7, True),
]
CELLS = {8: 1984, 16: 6192, 24: 14232, 32: 23424}


@pytest.mark.parametrize("name,resolution,env,pre,tol,cluster", WHOLE_SOLVE_CASES, ids=[c[0] for c in WHOLE_SOLVE_CASES])
def test_whole_solve_cg_iterate_leaves_the_residual_it_reports(name, resolution, env, pre, tol, cluster, monkeypatch):
    from fluidgym_amd.envs.cylinder_grid import build_domain, make_vortex_street_mesh

    _switches(monkeypatch, env)
    dom = build_domain(make_vortex_street_mesh(resolution), 0.01, batch=B)
    assert dom.n_cells == CELLS[resolution]
    if pre:
        dom.set_stall_limit(5000)
        ml = dom.set_pressure_multilevel()
        # (resolution 24: the table sizes the aggregate-owned layout needs, as test_aggregate_owned_onchip_cg_is_the_cell_ordered_one)
        assert ml == {"n4": 912, "n8": 228} if resolution == 24 else ml is not None, ml
    g = torch.Generator(device="cpu").manual_seed(11)
    dom.velocity.copy_((0.3 * torch.randn(dom.velocity.shape, generator=g)).to(dom.device))
    dom.velocity[:, 0] += 1.0
    dom.make_divergence_free(pressure_tol=tol, max_iterations=5000, pressure_project_mean=True)
    _held_step(name, dom, [0.01, 0.02], tol, 5000 if pre else 400, dict(advection_tol=tol), cluster=cluster)
    cfg = dom.config_dump()
    print(f"MB_CG_FORM {name}: cluster_on {cfg['cluster_on']} cluster_solves {cfg['cluster_solves']} cluster_fallbacks {cfg['cluster_fallbacks']}")
    assert (cfg["cluster_solves"] > 0) == cluster and cfg["cluster_fallbacks"] == 0, cfg
    dom.close()


@pytest.mark.parametrize("lib", ["f32", "f64"])
def test_one_cell_per_thread_cg_on_a_3d_mesh(lib, monkeypatch):
    """231 cells in 3-D, FG_MB_ONCHIP=0: k_mbc_ap<3, 1, 1> / k_mbc_update<1, false>, the instance tests/test_gpu_mbc_forms.py has no mesh
    for.  fp32 at the tolerance of test_piso_step_matches_oracle's CG cases; fp64 as test_fp64_piso_step_matches_the_oracle, and
    its velocity against the oracle's direct solves at that test's bound for skewed_pair_3d (1e-8)."""
    _switches(monkeypatch, {"FG_MB_ONCHIP": "0"})
    f64 = lib == "f64"
    dtype = torch.float64 if f64 else torch.float32
    spec = H.odd_channel_3d()
    d = spec.oracle()
    dom = spec.native(batch=B, dtype=dtype)
    assert dom.n_cells == 231 and dom.dims == 3
    dt = [0.05, 0.03]
    states = []
    for b in range(B):
        rng = np.random.default_rng(10 + b)
        u, p = 0.2 * rng.standard_normal((d.d, d.N)), 0.1 * rng.standard_normal(d.N)
        states.append((u, p - p.mean()))
        dom.velocity[b] = torch.as_tensor(u, dtype=dtype)
        dom.pressure[b] = torch.as_tensor(states[b][1], dtype=dtype)
    tol = 1e-13 if f64 else 2e-6
    _held_step(f"w1_3d.{lib}", dom, dt, tol, 400, dict(advection_tol=1e-13 if f64 else 1e-7), cap=20000 if f64 else 5000)
    if f64:
        u_gpu = dom.velocity.cpu().numpy()
        for b in range(B):
            u_ref, _ = d.piso_step(states[b][0], states[b][1], dt[b])
            err = float(np.abs(u_gpu[b] - u_ref).max() / np.abs(u_ref).max())
            print(f"MB_CG_W1_3D_ORACLE env {b}: velocity {err:.2e}")
            assert err < 1e-8, (b, err)
    dom.close()
