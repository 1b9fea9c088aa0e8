"""Every host driver of the single-block solvers (csrc/fg_bicgstab.hip: the five-kernel, two-kernel brick, two-kernel z-march and
six-launch Helmholtz forms of BiCGStab with their sub-batches, preconditioner modes, caps and masked envs; csrc/fg_jacobi.hip and
fg_linepre.hip: the on-chip, streaming and line sweeps with their back-off history; csrc/fg_poisson.hip and fg_fftcg.hip: the classic
and the fused pressure CG; the fp32 and the fp64 library) gives, bit for bit, what it gave when ``tests/golden/sb_driver_forms.npz``
was recorded (``tests/golden/make_golden_sb_driver_forms.py``, before the drivers were split into BicgRun + bicg_iterate_* / bicg_finish
and the poll round, the end of a solve and the sweep history were written once).  Launch order is part of the arithmetic here: a poll
that moves changes the iteration a solve ends in, so the record holds, for every solve on a handle, the SHA-256 of the result buffer
(3 velocity result, 7 scalar result, 6 pressure result), per system used_iterations / converged / is_finite and the bits of
final_residual, the returned status, and ``advection_jacobi_counts()``.  Every handle solves at least twice: the later solves are
placed by the iteration predictor (or the sweep history) that the earlier ones left behind.

The fixture is also asserted to show what it is there for: every uncapped Krylov case iterates (a system with used_iterations >= 3),
every capped case ends unconverged, the sub-batched groups end in different iterations, the give-up case is handed to BiCGStab, and
every other sweep case is settled by its sweeps.

Not covered: work vectors behind no buffer id (the recurrence's r, p, v, s, t: every later iterate and the residual words depend on
them), and the Jacobi speculation path, which tests/test_gpu_jacobi.py holds with ``torch.equal``."""
import contextlib
import ctypes
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.helpers import make_case

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "sb_driver_forms.npz")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("sha", "used", "conv", "fin", "res", "status", "counts")
# every switch a case may set: cleared before a case sets its own, so that a case never inherits one from the caller's environment
SWITCHES = ("FG_BICG_FUSED", "FG_BICG_SUB", "FG_BICG3", "FG_BICG3_MIX", "FG_BICG3_BXL", "FG_BICG_PFUSED", "FG_ADV_LINESWEEP", "FG_CG_FUSED",
            "FG_FCG_FIRST", "FG_FORCE_ZMARCH", "FG_ZMARCH_SB", "FG_POLL_WORDS", "FG_POLL_SPIN")


def _uniform_x(case):
    nx = len(case.widths[0])
    w = np.full(nx, np.float32(2.0 / nx), np.float32)
    case.widths[0] = w
    case.edges[0] = np.concatenate([[0.0], np.cumsum(w.astype(np.float64))])
    return case


def _wall_refined(case, ratio):
    ny = len(case.widths[1])
    half = ny // 2
    g = ratio ** (1.0 / max(half - 1, 1))
    w = np.concatenate([g ** np.arange(half), g ** np.arange(ny - half)[::-1]])
    w = (w / w.sum()).astype(np.float32)
    case.widths[1] = w
    case.edges[1] = np.concatenate([[0.0], np.cumsum(w.astype(np.float64))])
    return case


def _sweep_case(n, fixed, dims=2, seed=3, stretch=0.0):
    h = min(L / m for L, m in zip((2.0, 1.0, 1.5), n))
    return make_case(dims=dims, n=n, fixed_axes=fixed, B=3, seed=seed, stretch=stretch, nu=0.25 * h, vel_scale=0.5), h


GRIDS = {
    "a": lambda: make_case(dims=2, n=(32, 24), fixed_axes=(1,), B=3, seed=5, vel_scale=0.4, nu=0.03, n_scalars=1),
    "a2": lambda: make_case(dims=2, n=(32, 24), fixed_axes=(1,), B=2, seed=5, vel_scale=0.4, nu=0.03),
    "b": lambda: make_case(dims=2, n=(30, 17), fixed_axes=(0, 1), B=2, seed=6, vel_scale=0.4, nu=0.03),
    "p3": lambda: make_case(dims=3, n=(9, 8, 7), fixed_axes=(), B=2, seed=8, vel_scale=0.4, nu=0.03),
    "sub": lambda: make_case(dims=2, n=(64, 32), fixed_axes=(1,), B=5, seed=31, vel_scale=0.4, nu=0.03, n_scalars=1),
    "z": lambda: make_case(dims=3, n=(64, 16, 8), fixed_axes=(1,), B=2, seed=21, vel_scale=0.4, nu=0.03),
    "helm": lambda: _wall_refined(make_case(dims=2, n=(64, 32), fixed_axes=(1,), B=2, seed=9, n_scalars=1, stretch=0.0, vel_scale=0.4,
                                            nu=0.03), ratio=10.0),
    "giveup": lambda: make_case(dims=2, n=(256, 64), fixed_axes=(0, 1), B=2, seed=5, stretch=0.0, nu=0.05, vel_scale=0.5),
    "chan": lambda: _uniform_x(make_case(dims=2, n=(64, 24), fixed_axes=(0, 1), B=3, seed=2, stretch=0.3, with_source=True, vel_scale=0.3,
                                         through_flow_axis=0)),
    "chan3": lambda: make_case(dims=3, n=(20, 9, 6), fixed_axes=(1,), B=2, seed=4, vel_scale=0.3, with_source=True),
    "zm": lambda: make_case(dims=3, n=(64, 32, 32), fixed_axes=(1,), B=2, seed=4, vel_scale=0.3, with_source=True),
}

SUB_SCALE = (0.2, 1.0, 0.5, 1.5, 0.8)      # per-env velocity scaling of the sub-batch case: envs of different stiffness
CG, FDCG = 0, 4                            # FG_SOLVER_CG, FG_SOLVER_FDCG


def _adv(grid, env=None, lib="f32", scalar=False, pre=None, cap=5000, tols=(1e-7, 1e-7), start=(False, False), dt=0.08, scale=None):
    return dict(kind="adv", grid=grid, env=env or {}, lib=lib, scalar=scalar, pre=pre, cap=cap, tols=tols, start=start, dt=dt, scale=scale)


def _sweep(grid, dt, tol, env=None, pre=None, solves=2, jacobi=True):
    return dict(kind="sweep", grid=grid, env=env or {}, dt=dt, tol=tol, pre=pre, solves=solves, jacobi=jacobi)


def _press(grid, method, env=None, lib="f32", cap=5000, tol=1e-7, previous=False, child=False):
    return dict(kind="press", grid=grid, env=env or {}, lib=lib, method=method, cap=cap, tol=tol, previous=previous, child=child)


CASES = {}
for _f in ("0", "1"):
    _e = {"FG_BICG_FUSED": _f}
    CASES[f"bicg.f{_f}.a"] = _adv("a", _e)
    CASES[f"bicg.f{_f}.b"] = _adv("b", _e)
    CASES[f"bicg.f{_f}.a.scalar"] = _adv("a", _e, scalar=True)
    CASES[f"bicg.f{_f}.a.cap2"] = _adv("a", _e, cap=2)
    CASES[f"bicg.f{_f}.a.warm"] = _adv("a", _e, tols=(1e-6, 1e-5), start=(False, True))      # the second solve starts from the first's result
    CASES[f"bicg.f{_f}.a.masked"] = _adv("a", _e, dt=[0.08, 0.0, 0.08])
for _f in ("0", "2"):
    CASES[f"bicg3d.f{_f}"] = _adv("p3", {"FG_BICG_FUSED": _f})
CASES["bicg.sub2"] = _adv("sub", {"FG_BICG_SUB": "2"}, scale=SUB_SCALE)
CASES["bicg3.z4"] = _adv("z", {"FG_BICG3": "4"})
CASES["bicg3.z4.mix7"] = _adv("z", {"FG_BICG3": "4", "FG_BICG3_MIX": "7"})
CASES["bicg.pre1"] = _adv("a", pre=1)
CASES["bicg.pre4"] = _adv("a", pre=4)
for _f in ("0", "1"):
    CASES[f"helm.pf{_f}"] = _adv("helm", {"FG_BICG_PFUSED": _f}, pre=3)
CASES["f64.bicg.f0"] = _adv("a2", {"FG_BICG_FUSED": "0"}, lib="f64", tols=(1e-12, 1e-12))
CASES["f64.bicg.f1"] = _adv("a2", {"FG_BICG_FUSED": "1"}, lib="f64", tols=(1e-12, 1e-12))
CASES["f64.bicg.pre4"] = _adv("a2", lib="f64", pre=4, tols=(1e-12, 1e-12))

CASES["jac.128x64"] = _sweep(("jac", (128, 64), (0, 1)), None, None)
CASES["jac.256x37"] = _sweep(("jac", (256, 37), (1,)), None, None)
CASES["stream.36x18"] = _sweep(("stream", (36, 18), (0, 1), 2), None, None)
CASES["stream.24x20x8"] = _sweep(("stream", (24, 20, 8), (0, 1, 2), 3), None, None)
CASES["jac.giveup"] = _sweep("giveup", 0.05, 1e-6, solves=3)
CASES["linesweep"] = _sweep("helm", [0.002, 0.001], 2e-6 / 0.001, env={"FG_ADV_LINESWEEP": "1"}, pre=3, jacobi=False)

CASES["press.cg"] = _press("chan", CG)
CASES["press.fdcg.classic"] = _press("chan", FDCG, {"FG_CG_FUSED": "0"})
CASES["press.fdcg.first1"] = _press("chan", FDCG, {"FG_FCG_FIRST": "1"})
CASES["press.fdcg.first0"] = _press("chan", FDCG, {"FG_FCG_FIRST": "0"})
for _cap in (1, 3):
    CASES[f"press.fdcg.classic.cap{_cap}"] = _press("chan", FDCG, {"FG_CG_FUSED": "0"}, cap=_cap)
    CASES[f"press.fdcg.fused.cap{_cap}"] = _press("chan", FDCG, cap=_cap)
CASES["press.fdcg.previous"] = _press("chan", FDCG, previous=True)
CASES["press.fdcg.3d"] = _press("chan3", FDCG)
CASES["press.cg.zmarch"] = _press("zm", CG, {"FG_FORCE_ZMARCH": "8"}, tol=1e-6, child=True)      # (in a child process, as when the switch was read once per process; per handle now: test_gpu_switch_per_handle.py)
CASES["f64.press.fdcg"] = _press("chan", FDCG, lib="f64", tol=1e-12)

TRANSPORTS = {"words0": {"FG_POLL_WORDS": "0"}, "spin0": {"FG_POLL_SPIN": "0"}}
RUNS = [(name, None) for name in CASES] + [(name, t) for name in ("bicg.f1.a", "press.fdcg.first1") for t in TRANSPORTS]


def _record(ns, which, n_cells_shape, info, rc, sweeps):
    x = ns.buffer(which, n_cells_shape)
    c = ns.advection_jacobi_counts() if sweeps else {"settled_by_sweeps": 0, "handed_to_bicgstab": 0}
    return {"sha": np.frombuffer(hashlib.sha256(x.cpu().numpy().tobytes()).digest(), np.uint8),
            "used": np.array([i.used_iterations for i in info], np.int32),
            "conv": np.array([i.converged for i in info], np.uint8),
            "fin": np.array([i.is_finite for i in info], np.uint8),
            "res": np.array([i.final_residual for i in info], np.float64).view(np.uint64),
            "status": np.int32(rc), "counts": np.array([c["settled_by_sweeps"], c["handed_to_bicgstab"]], np.int64)}


def _solve_advection(ns, scalar, tol, cap):
    import torch

    from fluidgym_amd import _lib as L

    n = ns.B * (1 if scalar else ns.dims)
    info = ns._infos(n)
    rc = ns.lib.fg_solve_advection(ns.handle, int(scalar), 0, tol, cap, info, ctypes.c_void_p(torch.cuda.current_stream(ns.device).cuda_stream))
    L.check(rc, allow=(L.FG_ERR_NOT_CONVERGED, L.FG_ERR_NOT_FINITE))
    torch.cuda.synchronize()
    return rc, list(info)


def _solve_pressure(ns, method, tol, cap, previous):
    import torch

    from fluidgym_amd import _lib as L

    info = ns._infos(ns.B)
    rc = ns.lib.fg_solve_pressure(ns.handle, method, tol, cap, int(previous), info, ctypes.c_void_p(torch.cuda.current_stream(ns.device).cuda_stream))
    L.check(rc, allow=(L.FG_ERR_NOT_CONVERGED, L.FG_ERR_NOT_FINITE))
    torch.cuda.synchronize()
    return rc, list(info)


def _solve_here(spec):
    """The solves of one case on one fresh handle; the case's switches must be in the environment."""
    import torch

    dtype = torch.float64 if spec.get("lib") == "f64" else torch.float32
    grid, dt, tol = spec["grid"], spec.get("dt"), spec.get("tol")
    if isinstance(grid, tuple):      # the setup of the sweep tests: per env its own dt with CFL <= ~0.8, the tolerance scaled with 1 / dt
        kind, n, fixed = grid[:3]
        dims = grid[3] if kind == "stream" else 2
        case, h = _sweep_case(n, fixed, dims, seed=7 if kind == "stream" else 3, stretch=0.2 if kind == "stream" else 0.0)
        dt = [0.2 * h, 0.1 * h, 0.15 * h] if kind == "stream" else [0.2 * h, 0.4 * h, 0.1 * h]
        tol = 2e-7 / min(dt)
    else:
        case = GRIDS[grid]()
    ns = case.native(dtype=dtype)
    out = []
    if spec["kind"] == "adv":
        if spec["scale"] is not None:
            ns.velocity.mul_(torch.tensor(spec["scale"], dtype=dtype).view(-1, *([1] * (case.dims + 1))).to(ns.velocity.device))
        if spec["pre"] is not None:
            ns.set_advection_preconditioner(spec["pre"])
        scalar = spec["scalar"]
        shape = (case.B,) + case.shape if scalar else (case.B, case.dims) + case.shape
        for tol, from_result in zip(spec["tols"], spec["start"]):
            ns.set_advection_start(from_result)
            ns.setup_advection(spec["dt"], for_scalar=scalar, channel=0)
            rc, info = _solve_advection(ns, scalar, tol, spec["cap"])
            out.append(_record(ns, 7 if scalar else 3, shape, info, rc, False))
    elif spec["kind"] == "sweep":
        if spec["jacobi"]:
            ns.set_advection_jacobi(True)
        if spec["pre"] is not None:
            ns.set_advection_preconditioner(spec["pre"])
        ns.set_advection_start(False)
        for _ in range(spec["solves"]):
            ns.setup_advection(dt)
            rc, info = _solve_advection(ns, False, tol, 5000)
            out.append(_record(ns, 3, (case.B, case.dims) + case.shape, info, rc, True))
    else:
        dt = [0.02, 0.03, 0.025][:case.B]
        ns.setup_advection(dt)
        _solve_advection(ns, False, 1e-7 if dtype == torch.float32 else 1e-12, 5000)
        ns.setup_pressure_matrix()
        for k in range(2):
            ns.setup_pressure_rhs(dt)
            rc, info = _solve_pressure(ns, spec["method"], spec["tol"], spec["cap"], spec["previous"] and k == 1)
            out.append(_record(ns, 6, (case.B,) + case.shape, info, rc, False))
    ns.close()
    return {f: np.stack([r[f] for r in out]) for f in FIELDS}


def _child(name, path):
    """(entry of the child process of a case that runs in a process of its own)"""
    np.savez(path, **_solve_here(CASES[name]))


@contextlib.contextmanager
def _environment(setenv, delenv, env):
    for k in SWITCHES:
        delenv(k)
    for k, v in env.items():
        setenv(k, v)
    yield


def run_case(name, transport, setenv, delenv, tmp_dir):
    spec = CASES[name]
    env = dict(spec["env"], **(TRANSPORTS[transport] if transport else {}))
    with _environment(setenv, delenv, env):
        if not spec.get("child"):
            return _solve_here(spec)
        path = os.path.join(str(tmp_dir), name + ".npz")
        code = f"from tests import test_gpu_sb_driver_forms as T; T._child({name!r}, {path!r})"
        done = subprocess.run([sys.executable, "-c", code], env=dict(os.environ), cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-3000:]
        with np.load(path) as z:
            return {f: z[f] for f in FIELDS}


def shows_its_condition(name, g):
    """What the recorded data of a case must show for the case to be worth its place (asserted on the fixture)."""
    spec = CASES[name]
    used, conv, counts = g["used"], g["conv"], g["counts"]
    if spec["kind"] == "sweep":
        if name == "jac.giveup":
            return counts[-1, 1] >= 1
        return counts[-1, 0] >= 1
    if spec["cap"] < 5000:
        return not conv.any()
    if name == "bicg.sub2" and len(set(used[0].tolist())) < 2:
        return False
    return used.max() >= 3


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name,transport", RUNS)
def test_driver_reproduces_the_recorded_solves(name, transport, golden, monkeypatch, tmp_path):
    g = {f: golden[f"{name}.{f}"] for f in FIELDS}
    assert shows_its_condition(name, g), (name, g["used"].tolist(), g["conv"].tolist(), g["counts"].tolist())
    r = run_case(name, transport, monkeypatch.setenv, lambda k: monkeypatch.delenv(k, raising=False), tmp_path)
    print(name, transport, "used", r["used"].tolist(), "converged", r["conv"].tolist(), "status", r["status"].tolist(), "counts", r["counts"].tolist(),
          "residual", r["res"].view(np.float64).tolist())
    for f in ("status", "used", "conv", "fin", "counts", "res", "sha"):
        assert r[f].shape == g[f].shape and np.array_equal(r[f], g[f]), (name, transport, f, r[f].tolist(), g[f].tolist())
