"""Host side of the multilevel preconditioner in the fp64 build (no GPU): the policy switch, the one-argument behaviour of
``set_pressure_multilevel`` under the CPU stand-in, the entry points both libraries export, and the argument check of a host-only
fp64 handle."""
import ctypes

import numpy as np
import pytest
import torch

from fluidgym_amd import _lib as L

FG_ERR_INVALID_ARG = -1      # include/fluidgym_hip.h


def test_policy_exists_defaults_off_and_round_trips():
    from fluidgym_amd.simulation.policy import get_solver_policy, set_solver_policy

    assert get_solver_policy()["pressure_multilevel_fp64"] is False
    old = set_solver_policy(pressure_multilevel_fp64=True)
    try:
        assert old["pressure_multilevel_fp64"] is False
        assert get_solver_policy()["pressure_multilevel_fp64"] is True
        assert get_solver_policy()["pressure_multilevel"] is old["pressure_multilevel"]          # the neighbours are untouched
    finally:
        back = set_solver_policy(pressure_multilevel_fp64=old["pressure_multilevel_fp64"])
    assert back["pressure_multilevel_fp64"] is True and get_solver_policy()["pressure_multilevel_fp64"] is False
    with pytest.raises(KeyError):
        set_solver_policy(pressure_multilevel_f64=True)


def test_policy_is_documented_and_has_its_environment_switch():
    import fluidgym_amd.simulation.policy as P

    assert "``pressure_multilevel_fp64`` (default False)" in P.__doc__
    assert "FLUIDGYM_AMD_PRESSURE_MULTILEVEL_FP64" in P.__doc__
    import inspect
    assert 'os.environ.get("FLUIDGYM_AMD_PRESSURE_MULTILEVEL_FP64", "0")' in inspect.getsource(P)


def test_set_pressure_multilevel_keeps_its_one_argument_form_under_the_stub(monkeypatch):
    """tests/stub_mb.py replaces the method by ``lambda self, enable=True: None``: with the policy at its default the envs must
    keep calling it with no keyword (a cylinder env is built on the CPU through the stand-in)."""
    import inspect

    import fluidgym_amd
    import fluidgym_amd.simulation.multiblock as M
    from tests import stub_mb

    sig = inspect.signature(M.MultiBlockDomain.set_pressure_multilevel)
    assert list(sig.parameters) == ["self", "enable", "fp64"]
    assert sig.parameters["enable"].default is True
    assert sig.parameters["fp64"].default is False and sig.parameters["fp64"].kind is inspect.Parameter.KEYWORD_ONLY
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)   # FluidEnv.reset's guard; nothing here touches a GPU
    restore = stub_mb.install()
    try:
        # the stand-in takes no ``fp64`` keyword: building the env would raise a TypeError if the env base passed one
        env = fluidgym_amd.make("CylinderJet2D-easy-v0", num_envs=1, cuda_device="cpu", randomize_initial_state=False, initial_domain_steps=1)
        env.reset(seed=0)
        assert env._multilevel is None
        env.close()
    finally:
        restore()
    assert M.MultiBlockDomain.set_pressure_multilevel.__name__ == "set_pressure_multilevel"


@pytest.mark.parametrize("load", [L.load, L.load_f64])
def test_both_libraries_export_the_multilevel_entry_points(load):
    lib = load()
    for name in ("fg_mb_set_multilevel", "fg_mb_multilevel_apply", "fg_mb_multilevel_status", "fg_mb_debug_pressure_cg"):
        assert getattr(lib, name) is not None
    sig = (L.SIGNATURES if load is L.load else L.SIGNATURES_F64)["fg_mb_set_multilevel"][1]
    want = ctypes.c_float if load is L.load else ctypes.c_double
    assert sig[6] is ctypes.POINTER(want) and sig[7] is ctypes.POINTER(want) and sig[8] is want       # d4g, aci8, geom_diag_sum


@pytest.mark.parametrize("load", [L.load, L.load_f64])
def test_host_only_handle_refuses_the_tables_with_invalid_arg(load):
    """A handle created with device < 0 serves tables only: fg_mb_set_multilevel answers FG_ERR_INVALID_ARG in both builds (the
    fp64 build used to answer FG_ERR_UNSUPPORTED to every other handle), switch-only calls and status reads included."""
    lib = load()
    real = np.float32 if load is L.load else np.float64
    creal = ctypes.c_float if load is L.load else ctypes.c_double
    h = ctypes.c_void_p()
    L.check(lib.fg_mb_create(2, 1, -1, ctypes.byref(h)), lib=lib)
    try:
        nx, ny = 8, 4
        xs, ys = np.meshgrid(np.linspace(0.0, 2.0, nx + 1), np.linspace(0.0, 1.0, ny + 1))
        coords = np.ascontiguousarray(np.stack([xs, ys]), real)
        idx = ctypes.c_int32()
        L.check(lib.fg_mb_add_block(h, coords.ctypes.data_as(ctypes.POINTER(creal)), nx, ny, 1, ctypes.byref(idx)), lib=lib)
        L.check(lib.fg_mb_finalize(h), lib=lib)
        N = nx * ny
        i32 = ctypes.POINTER(ctypes.c_int32)
        a4 = np.zeros(N, np.int32); p4 = np.zeros(1, np.int32); rect = np.array([[0, nx, ny, nx]], np.int32)
        d4 = np.ones(1, real); aci = np.zeros((1, 1), real)
        rc = lib.fg_mb_set_multilevel(h, 1, 1, a4.ctypes.data_as(i32), p4.ctypes.data_as(i32), rect.ctypes.data_as(i32),
                                      d4.ctypes.data_as(ctypes.POINTER(creal)), aci.ctypes.data_as(ctypes.POINTER(creal)), 1.0, 1)
        assert rc == FG_ERR_INVALID_ARG
        assert lib.fg_mb_set_multilevel(h, 0, 0, None, None, None, None, None, 0.0, 0) == FG_ERR_INVALID_ARG
        out = (ctypes.c_int32 * 3)(7, 7, 7)
        L.check(lib.fg_mb_multilevel_status(h, out), lib=lib)
        assert list(out) == [0, 0, 0]
        z = (creal * N)()
        assert lib.fg_mb_multilevel_apply(h, z, z, None) == FG_ERR_INVALID_ARG
    finally:
        lib.fg_mb_destroy(h)


def test_switch_table_lists_the_new_switches():
    import os

    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "docs", "SWITCHES.md")).read()
    assert "`FLUIDGYM_AMD_PRESSURE_MULTILEVEL_FP64`" in text and "`FG_MB_PCG_KERNEL`" in text
