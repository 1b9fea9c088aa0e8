"""Every host driver of the multi-block solvers (csrc/fg_mb_krylov.hip: ``mb_bicgstab`` with its restart, verification round,
compacted launches, ILU / multilevel right preconditioners and fp64 refinement, ``mb_pressure_bicgstab``'s trial and back-off, ``mb_jacobi``
with its history, the chunked ``mb_cg``; csrc/fg_mb_onchip.hip and fg_mb_cluster.hip: the whole-solve CG and the cluster sweeps;
csrc/fg_mb_step.hip: the velocity and the pressure retry ladder of ``fg_mb_piso_step``; the fp32 and the fp64 library) gives, bit for
bit, what it gave when ``tests/golden/mb_driver_forms.npz`` was recorded (``tests/golden/make_golden_mb_driver_forms.py``, before the
drivers were split).  Launch order and poll placement are part of the arithmetic here: a poll that moves changes the iteration a solve
ends in.  Every case drives a fresh ``MultiBlockDomain`` through at least three steps, so that the later solves are placed by the
iteration predictors, the sweep history and the back-off words the earlier ones left, and records after every step the SHA-256 of the
velocity, the pressure and the velocity-result buffer, the four iteration counts and the status the step returns, ``env_status()``, the
48 words of ``solver_hints()``, ``ladder()``, ``solver_counters()``, ``advection_jacobi_counts()`` and ``multilevel_status()``.

The fixture is also asserted to show what it is there for (``shows_its_condition``): every uncapped Krylov case iterates (a system with
used_iterations >= 3), the capped case ends unconverged, the restart case goes beyond 100 iterations, the compaction case ends its
envs at least one poll apart, the forced-failure trial shows failures and a non-zero skip, the give-up cases are handed on and leave a
non-zero skip word, every settle case is settled by its sweeps, every ladder case increments exactly the rungs it names.

Not covered: the CG breakdown recovery (``k_mbs_recover``: nothing here provokes a breakdown), the cluster give-up (``-77``) path, and
the stderr traces; their code moved unchanged."""
import contextlib
import ctypes
import hashlib
import os

import numpy as np
import pytest

from tests import helpers_mb as H

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "mb_driver_forms.npz")
FIELDS = ("sha", "its", "status", "env_status", "hints", "ladder", "counters", "jacobi", "trial")
# every switch a case may set: cleared before a case sets its own, so that a case never inherits one from the caller's environment
SWITCHES = ("FG_MB_ML_FUSE", "FG_MB_ML_TRY_CAP", "FG_MB_COMPACT", "FG_MB_CL_JACOBI", "FG_MB_CLUSTER", "FG_MB_OC_AGG", "FG_MB_ONCHIP",
            "FG_MB_PCG_KERNEL", "FG_MB_RUNG_ILU", "FG_MB_BICG_VEC4", "FG_MB_BICG_FUSE", "FG_ADV_JACOBI", "FG_MB_CL_MAXCL", "FG_MB_CL_HALF",
            "FG_MB_CL_NEAR", "FG_MB_OC_RTG_NT", "FG_MB_OC_VARIANT", "FG_MB_TRACE", "FG_MB_TRACE_FAIL", "FG_POLL_WORDS", "FG_POLL_SPIN")

MESHES = {
    "chan": lambda: H.split_rotated_channel(40, 30),      # 1200 cells
    "odd": H.odd_channel,                                 # 77 cells: the one-cell-per-thread kernels
    "skew": H.skewed_pair,
    "ring": H.polar_ring,                                 # the multilevel tables fit
    "skew3d": H.skewed_pair_3d,                           # extrude(...) of the skewed pair
    "airfoil": lambda: H.airfoil_spec(div=4),
}
RUNGS = ("velocity_fp64", "velocity_preconditioned", "pressure_fp64", "pressure_cg")


def _case(mesh, dt, scale, env=None, lib="f32", steps=3, seed=3, ml=False, ml64=False, jacobi=False, warm=False, force=0, rungs=(),
          single=False, nan_env=None, uniform=False, cond="iterates", **kw):
    step = dict(advection_tol=1e-7, pressure_tol=1e-6)
    step.update(kw)
    return dict(mesh=mesh, dt=dt, scale=scale, env=env or {}, lib=lib, steps=steps, seed=seed, ml=ml, ml64=ml64, jacobi=jacobi, warm=warm,
                force=force, rungs=rungs, single=single, nan_env=nan_env, uniform=uniform, cond=cond, step=step)


DT3, SC3 = [0.05, 0.03, 0.02], [0.2, 0.4, 0.1]
CASES = {
    # ---- velocity BiCGStab (pressure: the on-chip CG these small meshes take by default)
    "bicg.chan": _case("chan", DT3, SC3),
    "bicg.odd": _case("odd", DT3, SC3),
    "bicg.3d": _case("skew3d", [0.05, 0.03], [0.2, 0.4], pressure_use_bicgstab=1),
    "bicg.cap2": _case("chan", DT3, SC3, max_iterations=2, cond="capped"),
    "bicg.masked": _case("chan", [0.05, 0.0, 0.02], SC3),
    "bicg.warm": _case("chan", DT3, SC3, warm=True),
    "bicg.single_step": _case("chan", 0.02, SC3, single=True),
    # ---- launched sweeps (no cluster tables on these meshes)
    # (fp32 sweeps: the tolerance scaled with 1 / dt as the right-hand side is, 2e-7 / min(dt) as in the single-block fixture)
    "sweeps.settle": _case("chan", [0.004, 0.002, 0.003], SC3, jacobi=True, env={"FG_MB_CL_JACOBI": "0"}, advection_tol=1e-4, cond="settles"),
    "sweeps.settle.3d": _case("skew3d", [0.002, 0.001], [0.2, 0.4], jacobi=True, advection_tol=2e-4, pressure_use_bicgstab=1, cond="settles"),
    "sweeps.giveup2": _case("chan", [0.004, 0.002, 0.003], SC3, jacobi=True, env={"FG_MB_CL_JACOBI": "0"}, nan_env=1, advection_tol=1e-4,
                           cond="gives_up"),
    "sweeps.giveup3": _case("chan", [0.5, 0.4, 0.3], SC3, jacobi=True, env={"FG_MB_CL_JACOBI": "0"}, steps=4, cond="gives_up"),
    # ---- the chunked CG and the kernel-form preconditioned CG on a small mesh
    "cg.chunked": _case("chan", DT3, SC3, env={"FG_MB_ONCHIP": "0"}, pressure_project_mean=True),
    "cg.chunked.odd": _case("odd", DT3, SC3, env={"FG_MB_ONCHIP": "0"}),
    "cg.onchip.ml": _case("ring", [0.05, 0.03], [0.2, 0.4], ml=True, pressure_project_mean=True),
    "cg.pcg_kernel": _case("ring", [0.05, 0.03], [0.2, 0.4], ml=True, env={"FG_MB_PCG_KERNEL": "1"}, pressure_project_mean=True),
    "cg.warm_then_cold": _case("chan", DT3, SC3, env={"FG_MB_ONCHIP": "0"}, pressure_warm_start=True, max_iterations=20, advection_tol=1e-3,
                               pressure_tol=1e-7, cond="capped"),
    # ---- compaction: one env of four much stiffer than the rest
    "compact": _case("chan", [0.02] * 4, [0.05, 0.05, 1.0, 0.05], pressure_use_bicgstab=1, pressure_tol=1e-5, cond="compacts"),
    # ---- the refined solve across a BICG_RESTART (airfoil, impulsive start)
    "refine.restart": _case("airfoil", [2e-3, 1e-3], [1.0, 0.6], uniform=True, pressure_use_bicgstab=2, pressure_project_mean=True,
                            pressure_tol=1e-7, cond="restarts"),
    # ---- the ladder (skewed pair; the option sets of test_retry_ladder_rungs_reproduce_the_plain_solve)
    "ladder.fp64": _case("skew", [0.02, 0.03], [0.2, 0.2], force=1, rungs=("velocity_fp64",), pressure_use_bicgstab=1, pressure_tol=2e-7,
                         solver_double_fallback=True, cond="ladder"),
    "ladder.pre.ilu": _case("skew", [0.02, 0.03], [0.2, 0.2], force=1, rungs=("velocity_preconditioned",), pressure_use_bicgstab=1,
                            pressure_tol=2e-7, bicg_precondition_fallback=True, cond="ladder"),
    "ladder.pre.cols": _case("skew", [0.02, 0.03], [0.2, 0.2], force=1, rungs=("velocity_preconditioned",), pressure_use_bicgstab=1,
                             pressure_tol=2e-7, bicg_precondition_fallback=True, env={"FG_MB_RUNG_ILU": "0"}, cond="ladder"),
    "ladder.fp64_then_pre": _case("skew", [0.02, 0.03], [0.2, 0.2], force=1 | 4, rungs=("velocity_fp64", "velocity_preconditioned"),
                                  pressure_use_bicgstab=1, pressure_tol=2e-7, solver_double_fallback=True, bicg_precondition_fallback=True,
                                  cond="ladder"),
    "ladder.pressure_fp64": _case("skew", [0.02, 0.03], [0.2, 0.2], force=2, rungs=("pressure_fp64",), pressure_use_bicgstab=1,
                                  pressure_tol=2e-7, solver_double_fallback=True, cond="ladder"),
    "ladder.pressure_cg": _case("skew", [0.02, 0.03], [0.2, 0.2], force=2, rungs=("pressure_cg",), pressure_use_bicgstab=1, pressure_tol=2e-7,
                                cond="ladder"),
    # ---- the fp64 library
    "f64.bicg": _case("chan", [0.05, 0.03], [0.2, 0.4], lib="f64", advection_tol=1e-12, pressure_tol=1e-11, pressure_use_bicgstab=1,
                      pressure_project_mean=True),
    "f64.refine": _case("ring", [0.05, 0.03], [0.2, 0.4], lib="f64", advection_tol=1e-12, pressure_tol=1e-11, pressure_use_bicgstab=2,
                        pressure_project_mean=True),
    "f64.pcg": _case("ring", [0.05, 0.03], [0.2, 0.4], lib="f64", ml64=True, advection_tol=1e-12, pressure_tol=1e-11, pressure_project_mean=True),
    "f64.sweeps": _case("chan", [0.004, 0.002], [0.2, 0.4], lib="f64", jacobi=True, advection_tol=1e-11, pressure_tol=1e-10, cond="settles"),
}
# ---- pressure BiCGStab with the multilevel right preconditioner, plain and refined, unfused and fused restriction
for _b in (1, 2):
    for _f in ("0", "2"):
        CASES[f"pbicg.ml.b{_b}.f{_f}"] = _case("ring", [0.05, 0.03, 0.04], SC3, ml=True, env={"FG_MB_ML_FUSE": _f}, pressure_use_bicgstab=_b,
                                              pressure_project_mean=True, pressure_tol=2e-6)
CASES["pbicg.ml.trial_fails"] = _case("ring", [0.05, 0.03, 0.04], SC3, ml=True, env={"FG_MB_ML_TRY_CAP": "2"}, pressure_use_bicgstab=1,
                                      pressure_project_mean=True, pressure_tol=2e-6, cond="trial_fails")
# ---- the resolution-24 cylinder mesh (8 x 8 aggregates): cluster sweeps + cluster CG, the aggregate-owned and the cell-ordered on-chip
# CG, the chunked CG and the kernel-form preconditioned CG
for _n, _e in (("cluster2", {"FG_MB_CLUSTER": "2"}), ("cluster0.agg1", {"FG_MB_CLUSTER": "0", "FG_MB_OC_AGG": "1"}),
               ("cluster0.agg0", {"FG_MB_CLUSTER": "0", "FG_MB_OC_AGG": "0"}), ("onchip0", {"FG_MB_CLUSTER": "0", "FG_MB_ONCHIP": "0"}),
               ("pcg_kernel", {"FG_MB_CLUSTER": "0", "FG_MB_PCG_KERNEL": "1"})):
    CASES[f"cyl.{_n}"] = _case("cyl24", [0.001, 0.0005, 0.0], None, env=_e, ml=True, jacobi=True, seed=11, advection_tol=5e-4,
                               pressure_project_mean=True, cond="settles")

TRANSPORTS = {"words0": {"FG_POLL_WORDS": "0"}, "spin0": {"FG_POLL_SPIN": "0"}}
# (case, transport, switches on top of the case's that are documented not to change results, live profiler's kernel class)
RUNS = [(name, None, None, None) for name in CASES]
RUNS += [(name, t, None, None) for name in ("bicg.chan", "pbicg.ml.b2.f2", "sweeps.settle", "cg.chunked") for t in TRANSPORTS]
RUNS += [("compact", None, "FG_MB_COMPACT=1", None), ("compact", None, "FG_MB_COMPACT=0", None)]
RUNS += [("cg.chunked", None, None, "k_mbc_ap"), ("cg.onchip.ml", None, None, "k_mbc_onchip"), ("cyl.cluster2", None, None, "k_mbc_onchip")]


def _domain(spec):
    import torch

    dtype = torch.float64 if spec["lib"] == "f64" else torch.float32
    B = len(spec["dt"]) if isinstance(spec["dt"], list) else len(spec["scale"])
    g = torch.Generator(device="cpu").manual_seed(spec["seed"])
    if spec["mesh"] == "cyl24":      # the state of tests/test_gpu_cluster.py, the envs scaled apart
        from fluidgym_amd.envs.cylinder_grid import build_domain, make_vortex_street_mesh

        dom = build_domain(make_vortex_street_mesh(24), 0.01, batch=B)
        dom.set_stall_limit(5000)
        v0 = 0.1 * torch.randn((1,) + tuple(dom.velocity.shape[1:]), generator=g)
        amp = torch.tensor([1.0, 0.7, 0.4][:B]).view(B, *([1] * (dom.velocity.dim() - 1)))
        dom.velocity.copy_((v0 * amp).to(dom.device))
        dom.velocity[:, 0] += 1.0
    else:
        dom = MESHES[spec["mesh"]]().native(batch=B, dtype=dtype)
        v = torch.randn(tuple(dom.velocity.shape), generator=g, dtype=torch.float64)
        if spec["uniform"]:      # impulsive start: the free stream everywhere
            v = torch.zeros_like(v)
            v[:, 0] = 1.0
        v = v * torch.tensor(spec["scale"], dtype=torch.float64).view(B, *([1] * (v.dim() - 1)))
        if spec["nan_env"] is not None:
            v[spec["nan_env"]] = float("nan")
        dom.velocity.copy_(v.to(dtype).to(dom.device))
    if spec["ml"]:
        assert dom.set_pressure_multilevel() is not None
    if spec["ml64"]:
        assert dom.set_pressure_multilevel(fp64=True) is not None
    if spec["mesh"] == "cyl24":
        dom.make_divergence_free(pressure_tol=1e-6, max_iterations=5000, pressure_project_mean=True)
    if spec["jacobi"]:
        dom.set_advection_jacobi(True)
    if spec["warm"]:
        dom.set_advection_start(True)
    return dom


def _step(dom, dt, corrector_steps=2, advect_non_ortho_steps=1, pressure_non_ortho_steps=1, advection_tol=1e-5, pressure_tol=1e-5,
          max_iterations=5000, pressure_use_bicgstab=0, pressure_warm_start=False, pressure_project_mean=False, solver_double_fallback=False,
          bicg_precondition_fallback=False):
    """``MultiBlockDomain.piso_step`` with all four counts and the status handed back."""
    import torch

    from fluidgym_amd import _lib as L

    dom._dt.copy_(torch.as_tensor(dt, dtype=dom.dtype).expand(dom.batch))
    opt = dom._step_options(corrector_steps, advect_non_ortho_steps, pressure_non_ortho_steps, advection_tol, pressure_tol, max_iterations,
                            pressure_use_bicgstab, pressure_warm_start, pressure_project_mean, 0.0, solver_double_fallback,
                            bicg_precondition_fallback)
    stats = (ctypes.c_int32 * 4)()
    rc = dom.lib.fg_mb_piso_step(dom.handle, ctypes.c_void_p(dom._dt.data_ptr()), ctypes.byref(opt), stats,
                                 ctypes.c_void_p(torch.cuda.current_stream(dom.device).cuda_stream))
    L.check(rc, allow=(L.FG_ERR_NOT_CONVERGED, L.FG_ERR_NOT_FINITE))
    torch.cuda.synchronize()
    return rc, list(stats)


def _sha(t):
    return np.frombuffer(hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).digest(), np.uint8)


def _record(dom, rc, its, force):
    from fluidgym_amd import _lib as L

    c = dom.solver_counters()
    counters = []
    for k in ("scalar", "velocity", "pressure0", "pressure1"):
        mean = c[k]["mean"]
        counters += [np.float64(-1.0 if mean is None else mean).view(np.int64), c[k]["max"], c[k]["systems"], c[k]["unconverged"]]
    counters.append(c["piso_steps"])
    j, t, lad = dom.advection_jacobi_counts(), dom.multilevel_status(), dom.ladder(force)      # (reading the rungs sets the test mask: keep the case's)
    return {"sha": np.stack([_sha(dom.velocity), _sha(dom.pressure), _sha(dom.buffer(L.FG_MB_BUF_VELOCITY_RESULT))]),
            "its": np.array(its, np.int32), "status": np.int32(rc), "env_status": dom.env_status().astype(np.int32),
            "hints": dom.solver_hints().numpy().astype(np.int32), "ladder": np.array([lad[k] for k in RUNGS], np.int64),
            "counters": np.array(counters, np.int64), "jacobi": np.array([j["settled_by_sweeps"], j["handed_to_bicgstab"]], np.int64),
            "trial": np.array([t["backoff"], t["attempts"], t["failed_attempts"]], np.int32)}


def _solve_here(spec, profile=None):
    """The steps of one case on one fresh domain; the case's switches must be in the environment."""
    dom = _domain(spec)
    dom.ladder(force_mask=spec["force"])
    if profile:
        dom.profile_enable(True)
    out = []
    for _ in range(spec["steps"]):
        if spec["single"]:
            _, ok, its = dom.single_step(spec["dt"], adaptive=True, **spec["step"])
            rc, its = 0 if ok else -5, [0] + list(its)
        else:
            rc, its = _step(dom, spec["dt"], **spec["step"])
        out.append(_record(dom, rc, its, spec["force"]))
    samples = dom.profile_read()[profile]["samples"] if profile else None
    dom.close()
    return {f: np.stack([r[f] for r in out]) for f in FIELDS}, samples


@contextlib.contextmanager
def _environment(setenv, delenv, env):
    for k in SWITCHES:
        delenv(k)
    for k, v in env.items():
        setenv(k, v)
    yield


def run_case(name, transport, extra, profile, setenv, delenv):
    spec = CASES[name]
    env = dict(spec["env"], **(TRANSPORTS[transport] if transport else {}))
    if extra:
        env.update([extra.split("=")])
    with _environment(setenv, delenv, env):
        return _solve_here(spec, profile)


def shows_its_condition(name, g):
    """What the recorded data of a case must show for the case to be worth its place (asserted on the fixture)."""
    spec = CASES[name]
    cond, its, status, hints, counters = spec["cond"], g["its"], g["status"], g["hints"], g["counters"]
    if cond == "capped":
        return bool((status == -5).all())                                  # FG_ERR_NOT_CONVERGED
    if its.max() < 3:                                                      # every uncapped case iterates
        return False
    if cond == "settles":
        return bool(g["jacobi"][-1, 0] > 0)
    if cond == "gives_up":
        backs_off = g["jacobi"][-1, 1] < len(its)      # later steps went past the sweeps: fewer hand-overs than steps
        return bool(g["jacobi"][-1, 1] > 0 and hints[:, 36:40].any() and (backs_off or name != "sweeps.giveup3"))
    if cond == "trial_fails":
        return bool(g["trial"][-1, 2] > 0 and hints[:, 34].any() and len(set(hints[:, 34].tolist())) > 1)
    if cond == "restarts":
        return bool(its[:, 2:].max() > 100)
    if cond == "compacts":
        # pressure0 after the first step: 4 systems; the slowest ends at least one poll (2 iterations) after the mean of the others
        mean, mx, n = counters[0, 8:9].view(np.float64)[0], counters[0, 9], counters[0, 10]
        return bool(n == 4 and (mx - mean) * n / (n - 1) >= 2.0)
    if cond == "ladder":
        return {k for k, v in zip(RUNGS, g["ladder"][-1]) if v > 0} == set(spec["rungs"])
    return True


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name,transport,extra,profile", RUNS)
def test_driver_reproduces_the_recorded_steps(name, transport, extra, profile, golden, monkeypatch):
    g = {f: golden[f"{name}.{f}"] for f in FIELDS}
    assert shows_its_condition(name, g), (name, g["its"].tolist(), g["status"].tolist(), g["jacobi"].tolist(), g["ladder"].tolist())
    r, samples = run_case(name, transport, extra, profile, monkeypatch.setenv, lambda k: monkeypatch.delenv(k, raising=False))
    print(name, transport, extra, profile, "its", r["its"].tolist(), "status", r["status"].tolist(), "env_status", r["env_status"].tolist(),
          "jacobi", r["jacobi"].tolist(), "ladder", r["ladder"].tolist(), "trial", r["trial"].tolist(), "samples", samples)
    for f in ("status", "its", "env_status", "ladder", "jacobi", "trial", "hints", "counters", "sha"):
        assert r[f].shape == g[f].shape and np.array_equal(r[f], g[f]), (name, transport, extra, f, r[f].tolist(), g[f].tolist())
    if profile:
        assert samples > 0, (name, profile, samples)
