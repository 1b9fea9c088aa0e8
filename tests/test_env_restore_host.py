"""Per-env restore without a GPU: the NumPy restatement against ``torch.roll(torch.flip(...))`` with the sign rule, the selection
builder's refusals (those of ``fg_env_restore_field``), the pinned draw order of ``reset_envs``, and the new symbols."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest
import torch

from fluidgym_amd import _lib as L
from fluidgym_amd.simulation.state_bank import SYMMETRIES, StateBank, build_selection, draw_reset_plan, normalize_envs
from tests.env_restore_ref import restore_ref, source_index, transform_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _torch_way(state, dims, fx, fz, sx, sz, signed):
    """The reference's sequence (rbc_env_base.py:335-362): mirrors with their sign change, then rolls."""
    t = torch.from_numpy(state.copy())
    if fx:
        t = torch.flip(t, dims=[-1])
        if signed:
            t[0] *= -1.0
    if fz:
        t = torch.flip(t, dims=[-3])
        if signed:
            t[2] *= -1.0
    t = torch.roll(t, shifts=sx, dims=-1)
    if dims == 3:
        t = torch.roll(t, shifts=sz, dims=-3)
    return t.numpy()


@pytest.mark.parametrize("dims,shape", [(2, (6, 20)), (2, (3, 7)), (3, (5, 4, 12))])
def test_reference_arithmetic_is_flip_then_roll_with_the_sign_rule(dims, shape):
    rng = np.random.default_rng(3)
    nx, nz = shape[-1], (shape[0] if dims == 3 else 1)
    for C, signed in ((dims, True), (1, False), (2, False)):
        state = rng.standard_normal((C,) + shape).astype(np.float32)
        state.flat[0] = 0.0          # a signed zero must come out as torch makes it
        shifts_z = (0, 1, nz - 1) if dims == 3 else (0,)
        for fx, fz, sx, sz in itertools.product((0, 1), (0, 1) if dims == 3 else (0,), (0, 1, nx // 2, nx - 1), shifts_z):
            mine = transform_state(state, dims, fx, fz, sx, sz, signed)
            ref = _torch_way(state, dims, fx, fz, sx, sz, signed)
            assert np.array_equal(_bits(mine), _bits(ref)), (C, fx, fz, sx, sz)
    # a face array (extent 1 along y) takes the same transform
    face = rng.standard_normal((dims,) + shape[:-2] + (1, nx)).astype(np.float32)
    assert np.array_equal(_bits(transform_state(face, dims, 1, 0, 3, 0, True)), _bits(_torch_way(face, dims, 1, 0, 3, 0, True)))
    assert source_index(5, 0, 0).tolist() == [0, 1, 2, 3, 4] and source_index(5, 1, 0).tolist() == [4, 3, 2, 1, 0]
    assert source_index(5, 0, 4).tolist() == [1, 2, 3, 4, 0] and source_index(5, 1, 4).tolist() == [3, 2, 1, 0, 4]


def test_restore_ref_leaves_the_other_envs_alone():
    rng = np.random.default_rng(4)
    dst = rng.standard_normal((5, 2, 6, 20)).astype(np.float32)
    bank = rng.standard_normal((3, 2, 6, 20)).astype(np.float32)
    out = restore_ref(dst, bank, 2, [1, 3], [2, 0], flip_x=[1, 0], shift_x=[19, 5], signed=True)
    for e in (0, 2, 4):
        assert np.array_equal(_bits(out[e]), _bits(dst[e]))
    assert np.array_equal(_bits(out[1]), _bits(_torch_way(bank[2], 2, 1, 0, 19, 0, True)))
    assert np.array_equal(_bits(out[3]), _bits(_torch_way(bank[0], 2, 0, 0, 5, 0, True)))


GRID2 = dict(batch=5, n_states=3, dims=2, nx=20, nz=1, periodic_x=True)
GRID3 = dict(batch=5, n_states=3, dims=3, nx=12, nz=5, periodic_x=True, periodic_z=True)


def test_selection_builder_fills_the_records():
    sel = build_selection([1, 3], [2, 0], flip_x=[1, 0], shift_x=[19, 0], **GRID2)
    assert len(sel) == 2 and ctypes.sizeof(L.FgEnvSel) == 24
    assert [(r.env, r.src, r.flip_x, r.flip_z, r.shift_x, r.shift_z) for r in sel] == [(1, 2, 1, 0, 19, 0), (3, 0, 0, 0, 0, 0)]
    sel = build_selection([0, 4], 1, flip_z=1, shift_z=[4, 0], shift_x=11, **GRID3)        # one value serves every chosen env
    assert [(r.env, r.src, r.flip_x, r.flip_z, r.shift_x, r.shift_z) for r in sel] == [(0, 1, 0, 1, 11, 4), (4, 1, 0, 1, 11, 0)]


@pytest.mark.parametrize("args,kw,grid", [
    (([5], 0), {}, GRID2),                                  # env out of range
    (([-1], 0), {}, GRID2),
    (([1], 3), {}, GRID2),                                  # source out of range
    (([1], -1), {}, GRID2),
    (([1, 1], 0), {}, GRID2),                               # an env twice
    (([0, 1, 2, 3, 4, 0], 0), {}, GRID2),                   # more records than envs
    (([], 0), {}, GRID2),
    (([1], 0), dict(shift_x=20), GRID2),                    # shift outside [0, n)
    (([1], 0), dict(shift_x=-1), GRID2),
    (([1], 0), dict(shift_z=5), GRID3),
    (([1], 0), dict(flip_x=2), GRID2),                      # a flip is 0 or 1
    (([1], 0), dict(flip_x=1), {**GRID2, "periodic_x": False}),      # an axis that is not periodic
    (([1], 0), dict(shift_x=1), {**GRID2, "periodic_x": False}),
    (([1], 0), dict(flip_z=1), {**GRID3, "periodic_z": False}),
    (([1], 0), dict(shift_z=1), {**GRID3, "periodic_z": False}),
    (([1], 0), dict(flip_z=1), GRID2),                      # z on a 2-D grid
    (([1], 0), dict(shift_z=1), {**GRID2, "nz": 4}),
    (([1, 2], [0]), dict(shift_x=[1, 2, 3]), GRID2),        # a column of another length
])
def test_selection_builder_refuses_what_the_library_refuses(args, kw, grid):
    with pytest.raises(ValueError):
        build_selection(*args, **kw, **grid)


def test_normalize_envs():
    assert normalize_envs([3, 0, 2], 5) == [0, 2, 3]
    assert normalize_envs(np.array([False, True, False, True, False]), 5) == [1, 3]
    assert normalize_envs(torch.tensor([True, False, False]), 3) == [0]
    for bad in ([5], [-1], [1, 1], [], np.array([True, False]), [0.5]):
        with pytest.raises(ValueError):
            normalize_envs(bad, 5)


def test_draw_order_of_reset_envs_is_pinned():
    """Per chosen env in ascending index order: the source (more than one state), then flip_x, flip_z, shift_x, shift_z -- those the
    family has.  The numbers are those of numpy.random.default_rng, drawn here once and written down."""
    rng = np.random.default_rng(7)
    plan = draw_reset_plan(rng, [3, 0, 2], 4, ("flip_x", "shift_x"), 20, 1, True)
    assert plan == {"env": [0, 2, 3], "src": [3, 2, 0], "flip_x": [1, 0, 1], "flip_z": [0, 0, 0], "shift_x": [12, 15, 6], "shift_z": [0, 0, 0]}
    assert int(rng.integers(0, 1000)) == 912          # nine numbers were drawn, no more
    # the same numbers by hand: the order IS the contract
    rng = np.random.default_rng(7)
    by_hand = []
    for _ in range(3):
        by_hand.append((int(rng.integers(0, 4)), int(rng.uniform(0.0, 1.0) > 0.5), int(rng.integers(0, 20))))
    assert by_hand == list(zip(plan["src"], plan["flip_x"], plan["shift_x"]))
    rng = np.random.default_rng(11)
    plan = draw_reset_plan(rng, [1, 4], 3, SYMMETRIES, 12, 5, True)
    assert plan == {"env": [1, 4], "src": [0, 0], "flip_x": [0, 0], "flip_z": [1, 1], "shift_x": [1, 6], "shift_z": [3, 0]}
    assert int(rng.integers(0, 1000)) == 542
    # a bank of one draws no source; without randomize nothing is drawn at all
    rng = np.random.default_rng(11)
    plan = draw_reset_plan(rng, [1, 4], 1, SYMMETRIES, 12, 5, True)
    assert plan["src"] == [0, 0] and plan["shift_x"] == [7, 4] and plan["shift_z"] == [3, 4]
    rng, fresh = np.random.default_rng(11), np.random.default_rng(11)
    plan = draw_reset_plan(rng, [1, 4], 3, SYMMETRIES, 12, 5, False)
    assert all(v == [0, 0] for k, v in plan.items() if k != "env")
    assert int(rng.integers(0, 1000)) == int(fresh.integers(0, 1000))
    with pytest.raises(ValueError):
        draw_reset_plan(rng, [0], 1, ("flip_y",), 12)


def test_state_bank_from_snapshots():
    mk = lambda B, k: {"velocity": torch.full((B, 2, 3, 4), float(k)), "pressure": torch.full((B, 1, 3, 4), float(k)),
                       "bvel": {2: torch.full((B, 2, 1, 4), float(k)), 3: torch.full((B, 2, 1, 4), float(k))}, "bscal": {},
                       "solver_hints": [0] * 12}
    snaps = [mk(2, 0), {"domain": mk(2, 1), "n_steps": 3}]
    for s in snaps:
        s_dom = s.get("domain", s)
        s_dom["velocity"][1] += 0.5
    bank = StateBank(snaps)                      # every env of every snapshot
    assert len(bank) == 4 and bank.fields["velocity"][:, 0, 0, 0].tolist() == [0.0, 0.5, 1.0, 1.5]
    assert sorted(bank.bvel) == [2, 3] and bank.bvel[2].shape == (4, 2, 1, 4) and bank.bscal == {}
    bank = StateBank(snaps, env=1)               # env 1 of each
    assert bank.size == 2 and bank.fields["velocity"][:, 0, 0, 0].tolist() == [0.5, 1.5]
    assert all(t.is_contiguous() for t in bank.fields.values())
    with pytest.raises(ValueError):
        StateBank([])
    with pytest.raises(ValueError):
        StateBank([mk(1, 0), {k: v for k, v in mk(1, 0).items() if k != "pressure"}])


def test_new_symbols_are_declared_typed_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fluidgym_hip.h")).read(), flags=re.S)
    names = ("fg_env_restore_field", "fg_env_reset_solver_state", "fg_mb_env_restore_field", "fg_mb_env_reset_solver_state")
    for name in names:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert name in L.SIGNATURES and name in L.SIGNATURES_F64
    assert re.search(r"typedef struct fg_env_sel\s*\{[^}]*env, src;[^}]*flip_x, flip_z;[^}]*shift_x, shift_z;[^}]*\}\s*fg_env_sel;", text)
    assert [n for n, _ in L.FgEnvSel._fields_] == ["env", "src", "flip_x", "flip_z", "shift_x", "shift_z"]
    assert L.SIGNATURES["fg_env_restore_field"][1] == [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int32,
                                                       ctypes.POINTER(L.FgEnvSel), ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p]
    for lib in (L.load(), L.load_f64()):         # a kernel of both builds, not a stub of the fp64 one
        for name in names:
            assert hasattr(lib, name), name
        # a multi-block handle has no per-env restore; a null handle is an argument error (no launch either way)
        assert lib.fg_mb_env_restore_field(None, 0, None, 1, None, 1, 0, None) == L.FG_ERR_UNSUPPORTED
        assert lib.fg_mb_env_reset_solver_state(None, None, 1, None) == L.FG_ERR_UNSUPPORTED
        assert lib.fg_env_restore_field(None, 0, None, 1, None, 1, 0, None) == L.FG_ERR_INVALID_ARG
        assert lib.fg_env_reset_solver_state(None, None, 1, None) == L.FG_ERR_INVALID_ARG
    stubs = open(os.path.join(ROOT, "fluidgym_amd", "csrc", "fg_f64_stubs.hip")).read()
    assert "fg_env_restore_field" not in stubs and "fg_env_reset_solver_state" not in stubs
