"""CPU-side checks of the baseline controllers (``fluidgym_amd/baselines.py``, ``csrc/fg_baselines.hip``): the ABI
of the two entry points and their argument checks (which answer before any launch, without a GPU), the properties of the NumPy
restatement the GPU tests compare against, and the controller classes on envs that never touch the GPU."""
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import fluidgym_amd
from fluidgym_amd import _lib as L
from fluidgym_amd.baselines import OppositionControl, PDControl
from fluidgym_amd.envs.rbc import RBCEnv2D
from tests import baselines_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fg_baseline_opposition", "fg_baseline_pd")


# ------------------------------------------------------------------------------------------------ ABI and argument checks
def test_both_libraries_export_the_entry_points():
    header = open(os.path.join(ROOT, "include", "fluidgym_hip.h")).read()
    mk = open(os.path.join(ROOT, "fluidgym_amd", "csrc", "Makefile")).read()
    assert all("fg_baselines.hip" in line for line in mk.splitlines() if line.startswith(("SRCS =", "F64_SRCS =")))
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header)
        assert name in L.SIGNATURES and name in L.SIGNATURES_F64
        assert hasattr(L.load(), name) and hasattr(L.load_f64(), name)
    assert fluidgym_amd.OppositionControl is OppositionControl and fluidgym_amd.PDControl is PDControl
    assert callable(fluidgym_amd.run_baseline_episodes)


def _int32s(*v):
    return (ctypes.c_int32 * len(v))(*v)


def _doubles(*v):
    return (ctypes.c_double * len(v))(*v)


@pytest.mark.parametrize("lib_name", ["fp32", "fp64"])
def test_opposition_argument_checks_answer_before_any_launch(lib_name):
    lib = L.load() if lib_name == "fp32" else L.load_f64()
    one = ctypes.c_void_p(64)                  # never dereferenced: every call below fails its argument checks first
    rows, gain = _int32s(3, 12), _doubles(-1.0, 1.0)
    # (v, batch_stride, batch, nz, ny, nx, rows, gain, n_walls, actor, action)
    good = [one, 16 * 16 * 8 * 3, 2, 8, 16, 16, rows, gain, 2, 2, one]
    bad = {
        "null field": {0: None}, "null rows": {6: None}, "null gain": {7: None}, "null action": {10: None},
        "batch < 1": {2: 0}, "actor < 1": {9: 0}, "actor does not divide nx": {9: 3, 3: 9}, "actor does not divide nz": {9: 4, 3: 6},
        "n_walls 0": {8: 0}, "n_walls 3": {8: 3}, "row below 0": {6: _int32s(-1, 12)}, "row at ny": {6: _int32s(3, 16)},
        "second row outside": {6: _int32s(3, 99)}, "non-positive extent": {4: 0}, "short batch stride": {1: 16 * 16 * 8 - 1},
    }
    for what, change in bad.items():
        args = list(good)
        for k, v in change.items():
            args[k] = v
        assert lib.fg_baseline_opposition(*args, None) == L.FG_ERR_INVALID_ARG, what
        assert b"fg_baseline_opposition" in lib.fg_last_error(), what
    # a row that only the unused second wall would break is not looked at with one wall
    one_wall = list(good)
    one_wall[6], one_wall[8], one_wall[0] = _int32s(3, 99), 1, None
    assert lib.fg_baseline_opposition(*one_wall, None) == L.FG_ERR_INVALID_ARG and b"null field" in lib.fg_last_error()


@pytest.mark.parametrize("lib_name", ["fp32", "fp64"])
def test_pd_argument_checks_answer_before_any_launch(lib_name):
    lib = L.load() if lib_name == "fp32" else L.load_f64()
    one = ctypes.c_void_p(64)
    # (v, batch_stride, batch, nz, ny, nx, seg, wy, kp, kd_over_dt, e_state, first, tickets, action)
    good = [one, 32 * 20 * 2, 3, 1, 20, 32, 8, one, 970.0, 2000.0, one, one, one, one]
    bad = {
        "null field": {0: None}, "null wy": {7: None}, "null e_state": {10: None}, "null first": {11: None}, "null tickets": {12: None},
        "null action": {13: None}, "batch < 1": {2: 0}, "seg < 1": {6: 0}, "seg does not divide nx": {6: 5},
        "seg does not divide nz": {3: 12, 1: 32 * 20 * 12}, "non-positive extent": {5: 0}, "short batch stride": {1: 32 * 20 - 1},
    }
    for what, change in bad.items():
        args = list(good)
        for k, v in change.items():
            args[k] = v
        assert lib.fg_baseline_pd(*args, None) == L.FG_ERR_INVALID_ARG, what
        assert b"fg_baseline_pd" in lib.fg_last_error(), what


# ------------------------------------------------------------------------------------------------ the restatement
def _field(seed, shape=(2, 8, 16, 12)):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def test_opposition_action_sums_to_zero_per_wall():
    v = _field(0)
    a = R.opposition_action(v, [3, 12], [-1.0, 1.0], 2)
    assert a.shape == (2, 2, 6, 4)
    assert np.abs(a.sum(axis=(2, 3))).max() <= 24 * 8 * 2.0 ** -52 * np.abs(v).max()


def test_opposition_action_axes_are_x_then_z():
    """v = sin(2 pi x / L), the same at every z: constant along the naz axis, varying along nax (an x / z transposition would swap it)."""
    nz, ny, nx = 8, 4, 12
    v = np.broadcast_to(np.sin(2 * np.pi * (np.arange(nx) + 0.5) / nx), (1, nz, ny, nx))
    a = R.opposition_action(v, [1], [-1.0], 2)[0, 0]                    # [nax, naz]
    assert a.shape == (6, 4)
    assert np.abs(a - a[:, :1]).max() <= 1e-15
    assert np.ptp(a[:, 0]) > 1.0


@pytest.mark.parametrize("alpha", [1.0, 0.5])
def test_restated_action_through_the_envs_own_control_is_minus_alpha_v_prime_on_both_walls(alpha):
    env = fluidgym_amd.make("TCFSmall3D-both-easy-v0", cuda_device=torch.device("cpu"), num_envs=2, resolution_y=16, resolution_x=12,
                            resolution_z=8, actor_size=2)
    env.scale_actions = False
    v = _field(1).astype(np.float64)                                    # [B, Z, Y, X]
    rows = [3, 12]
    a = R.opposition_action(v, rows, [-alpha, alpha], 2)
    # what TCF3DBothEnv._apply_action writes on the walls: repeat_interleave, transpose, the top wall negated
    walls = [env._action_to_control(torch.as_tensor(a[:, 0])).numpy(), -env._action_to_control(torch.as_tensor(a[:, 1])).numpy()]
    for r, wall in zip(rows, walls):
        plane = v[:, :, r, :]
        fluct = plane - plane.mean(axis=(1, 2), keepdims=True)
        patch = fluct.reshape(2, 4, 2, 6, 2).mean(axis=(2, 4))          # [B, Z / 2, X / 2]
        want = -alpha * np.repeat(np.repeat(patch, 2, axis=1), 2, axis=2)
        assert wall.shape == want.shape == (2, 8, 12)
        assert np.abs(wall - want).max() <= 1e-14


def test_pd_restatement_derivative_and_reset():
    rng = np.random.default_rng(2)
    wy = rng.uniform(0.5, 1.5, 10)
    wy /= wy.sum()
    v1, v2, v3 = (rng.standard_normal((3, 1, 10, 16)) for _ in range(3))
    E1, E2, E3 = (R.pd_energy(v, wy, 4) for v in (v1, v2, v3))
    assert E1.shape == (3, 1, 4)
    assert np.allclose(R.pd_energy(np.ones((3, 1, 10, 16)), wy, 4), 1.0, rtol=1e-14)       # the weights sum to 1
    c = R.PDController(3, 970.0, 40.0)
    assert np.array_equal(c.action(v1, wy, 4), -(970.0 * E1))                              # first call: no derivative
    assert np.allclose(c.action(v2, wy, 4), -(970.0 * E2 + 40.0 * (E2 - E1)), rtol=1e-14)
    c.reset(envs=[1])
    a3 = c.action(v3, wy, 4)
    assert np.array_equal(a3[1], -(970.0 * E3[1]))                                         # env 1 alone lost its derivative
    assert np.allclose(a3[[0, 2]], -(970.0 * E3 + 40.0 * (E3 - E2))[[0, 2]], rtol=1e-14)
    assert not np.array_equal(a3[0], -(970.0 * E3[0]))
    # 3-D: heaters are [z, x]
    v = rng.standard_normal((2, 8, 5, 8))
    E = R.pd_energy(v, np.full(5, 0.2), 4)
    assert E.shape == (2, 2, 2) and np.isclose(E[1, 1, 0], v[1, 4:, :, :4].mean(), rtol=1e-13)


# ------------------------------------------------------------------------------------------------ the controller classes
def test_controllers_refuse_the_other_env_family():
    tcf = fluidgym_amd.make("TCFSmall3D-bottom-easy-v0", cuda_device=torch.device("cpu"), resolution_y=16, resolution_x_z=16)
    rbc = fluidgym_amd.make("RBC2D-easy-v0", cuda_device=torch.device("cpu"), n_heaters=4, resolution=8)
    with pytest.raises(TypeError, match="OppositionControl"):
        OppositionControl(rbc)
    with pytest.raises(TypeError, match="PDControl"):
        PDControl(tcf)
    with pytest.raises(TypeError):
        OppositionControl(object())
    ctrl = OppositionControl(tcf)
    assert ctrl.n_walls == 1 and ctrl.alpha == 1.0 and ctrl.y_plus == 15.0
    with pytest.raises(RuntimeError, match="scale_actions"):
        ctrl.action()                                                   # scaled actions are refused before anything else
    tcf.scale_actions = False
    with pytest.raises(RuntimeError, match="reset"):
        ctrl.action()
    pd = PDControl(rbc)
    assert (pd.kp, pd.kd) == (970.0, 2000.0)
    pd.reset()                                                          # before the first reset of the env: nothing to forget
    with pytest.raises(RuntimeError, match="reset"):
        pd.action()


class StubRBC(RBCEnv2D):
    """An RBC env that has "been reset" without a solver: the members ``PDControl`` reads, on CPU tensors."""

    def __init__(self, num_envs=3, ny=6, n_heaters=4, width=2):
        self._num_envs, self._heater_width, self._n_heaters, self._step_length = num_envs, width, n_heaters, 0.5
        self._domain = object()
        self._block = SimpleNamespace(velocity=torch.zeros(num_envs, 2, ny, n_heaters * width),
                                      edges=[np.linspace(0, 1, n_heaters * width + 1), np.array([0.0, 0.1, 0.3, 0.5, 0.7, 0.9, 1.0])])


def test_pd_control_reset_names_envs():
    ctrl = PDControl(StubRBC())
    wy, e_state, first, tickets = ctrl._bind()
    assert np.allclose(wy.numpy(), [0.1, 0.2, 0.2, 0.2, 0.2, 0.1]) and wy.dtype == torch.float64
    assert e_state.shape == (3, 1, 4) and first.tolist() == [1, 1, 1] and tickets.tolist() == [0, 0, 0]
    first.zero_()
    ctrl.reset(envs=[1])
    assert first.tolist() == [0, 1, 0]
    ctrl.reset(envs=np.array([True, False, False]))
    assert first.tolist() == [1, 1, 0]
    first.zero_()
    ctrl.reset()
    assert first.tolist() == [1, 1, 1]
    with pytest.raises(ValueError):
        ctrl.reset(envs=[3])
