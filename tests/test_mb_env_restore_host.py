"""Per-env restore of the multi-block handles without a GPU: the symbol in both libraries, every refusal of ``fg_mb_restore_envs`` from
host-only handles (``fg_mb_create(d, B, -1)``), the NumPy restatement against per-block ``torch.roll(torch.flip(...))``,
``span_symmetry``, ``MeshStateBank`` and the refusing stubs of ``ParallelFluidEnv``.

Not exercised here: ``FG_ERR_UNSUPPORTED`` for noise with more than 2^26 cells -- a handle of that size takes gigabytes of host tables."""
import ctypes
import itertools
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from fluidgym_amd import _lib as L
from fluidgym_amd.simulation.mb_state_bank import MeshStateBank, span_symmetry
from tests.mb_env_restore_ref import restore_ref

B = 4


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _coords(dims, nx, ny, nz, dtype):
    x, y = np.linspace(0, 1, nx + 1), np.linspace(0, 1, ny + 1)
    if dims == 2:
        return np.ascontiguousarray(np.stack(np.meshgrid(x, y, indexing="xy")).astype(dtype))                # [2, ny+1, nx+1]
    z = np.linspace(0, 1, nz + 1)
    Z, Y, X = np.meshgrid(z, y, x, indexing="ij")
    return np.ascontiguousarray(np.stack([X, Y, Z]).astype(dtype))                                           # [3, nz+1, ny+1, nx+1]


def _handle(lib, real, dims, blocks, periodic_z=(), finalize=True):
    """A host-only handle of ``blocks`` = [(nx, ny, nz)], unconnected (every face FIXED but the periodic ones)."""
    h = ctypes.c_void_p()
    assert lib.fg_mb_create(dims, B, -1, ctypes.byref(h)) == 0
    for nx, ny, nz in blocks:
        c = _coords(dims, nx, ny, nz, np.float64 if real is ctypes.c_double else np.float32)
        assert lib.fg_mb_add_block(h, c.ctypes.data_as(ctypes.POINTER(real)), nx, ny, nz, None) == 0
    for b in periodic_z:
        assert lib.fg_mb_make_periodic(h, b, 2) == 0
    if finalize:
        assert lib.fg_mb_finalize(h) == 0
    return h


LIBS = [("f32", L.load, ctypes.c_float), ("f64", L.load_f64, ctypes.c_double)]


@pytest.mark.parametrize("name,load,real", LIBS, ids=[n for n, _, _ in LIBS])
def test_both_libraries_export_the_entry_and_refuse_by_code(name, load, real):
    lib = load()
    assert hasattr(lib, "fg_mb_restore_envs")
    assert "fg_mb_restore_envs" in L.SIGNATURES and "fg_mb_restore_envs" in L.SIGNATURES_F64
    bank = (real * 8)()                  # never read: every call below ends before a launch
    bp = ctypes.cast(bank, ctypes.c_void_p)
    sel = lambda *recs: (L.FgEnvSel * len(recs))(*[L.FgEnvSel(*r) for r in recs])
    ep = (ctypes.c_uint32 * B)()
    noise = lambda su, sp: ctypes.byref(L.FgMbResetNoise(7, su, sp, ep))
    call = lambda h, s, n=None, S=2, nz=None, bv=bp, bpr=bp, bb=bp: lib.fg_mb_restore_envs(h, bv, bpr, bb, S, s, len(s) if n is None else n, nz, None)
    ok = sel((1, 0, 0, 0, 0, 0))

    h2 = _handle(lib, real, 2, [(3, 4, 1)])
    h3 = _handle(lib, real, 3, [(3, 4, 3), (4, 3, 3)], periodic_z=(0, 1))
    h3_open = _handle(lib, real, 3, [(3, 4, 3), (4, 3, 3)], periodic_z=(0,))          # one block not z-periodic
    h3_mixed = _handle(lib, real, 3, [(3, 4, 3), (4, 3, 4)], periodic_z=(0, 1))       # two values of nz
    raw = _handle(lib, real, 2, [(3, 4, 1)], finalize=False)
    try:
        bad = L.FG_ERR_INVALID_ARG
        # null handle, selection, banks; S < 1
        assert call(None, ok) == bad
        assert lib.fg_mb_restore_envs(h2, bp, bp, bp, 2, None, 1, None, None) == bad
        assert call(h2, ok, bv=None) == bad and call(h2, ok, bpr=None) == bad and call(h2, ok, bb=None) == bad
        assert call(h2, ok, S=0) == bad
        # n_sel outside 1..B
        assert call(h2, ok, n=0) == bad and call(h2, sel(*[(e % B, 0, 0, 0, 0, 0) for e in range(B + 1)])) == bad
        # an env out of range or named twice; src outside [0, S)
        assert call(h2, sel((B, 0, 0, 0, 0, 0))) == bad and call(h2, sel((-1, 0, 0, 0, 0, 0))) == bad
        assert call(h2, sel((1, 0, 0, 0, 0, 0), (1, 1, 0, 0, 0, 0))) == bad
        assert call(h2, sel((1, 2, 0, 0, 0, 0))) == bad and call(h2, sel((1, -1, 0, 0, 0, 0))) == bad
        # flip_x / shift_x; a flip that is not 0 or 1; shift_z outside [0, nz)
        assert call(h3, sel((1, 0, 1, 0, 0, 0))) == bad and call(h3, sel((1, 0, 0, 0, 1, 0))) == bad
        assert call(h3, sel((1, 0, 0, 2, 0, 0))) == bad and call(h3, sel((1, 0, 0, -1, 0, 0))) == bad
        assert call(h3, sel((1, 0, 0, 0, 0, 3))) == bad and call(h3, sel((1, 0, 0, 0, 0, -1))) == bad
        # flip_z / shift_z on a handle that is not 3-D with every block z-periodic and of one nz
        for h in (h2, h3_open, h3_mixed):
            assert call(h, sel((1, 0, 0, 1, 0, 0))) == bad and call(h, sel((1, 0, 0, 0, 0, 1))) == bad
        # a sigma that is negative or not finite
        for su, sp in ((-1.0, 0.0), (0.0, -1e-9), (math.inf, 0.0), (0.0, math.nan)):
            assert call(h3, ok, nz=noise(su, sp)) == bad
        assert b"sigma" in lib.fg_last_error()
        # valid calls end at the bound-field check, with and without noise and a z symmetry; an unfinalised handle likewise
        unbound = L.FG_ERR_NOT_BOUND
        assert call(h2, ok) == unbound and call(h2, ok, nz=noise(0.025, 0.025)) == unbound
        assert call(h3, sel((0, 1, 0, 1, 0, 2), (3, 0, 0, 0, 0, 1)), nz=noise(0.0, 0.01)) == unbound
        assert call(h3_open, ok) == unbound and call(h3_mixed, ok) == unbound
        assert call(raw, ok) == unbound
        # the two older multi-block entries keep refusing
        assert lib.fg_mb_env_restore_field(h3, 0, None, 1, None, 1, 0, None) == L.FG_ERR_UNSUPPORTED
    finally:
        for h in (h2, h3, h3_open, h3_mixed, raw):
            assert lib.fg_mb_destroy(h) == 0


def _fake_blocks(sizes, fixed_faces):
    """Blocks as the restatement reads them, laid out as ``fg_mb_finalize`` lays them out: cells in block order, slots in (block, face) order."""
    blocks, off, slot = [], 0, 0
    for size in sizes:
        n = int(np.prod(size))
        slots = []
        for f in range(2 * len(size)):
            if f in fixed_faces:
                slots.append(slot)
                slot += n // size[f >> 1]
            else:
                slots.append(-1)
        blocks.append(SimpleNamespace(cell_offset=off, size=tuple(size), boundary_slot0=slots))
        off += n
    return blocks, off, slot


def test_restatement_is_roll_of_flip_per_block_and_face():
    rng = np.random.default_rng(5)
    nz, sizes = 3, [(5, 6, 3), (4, 3, 3)]
    blocks, N, NB = _fake_blocks(sizes, fixed_faces=(0, 3))
    bank_v, bank_p, bank_b = rng.standard_normal((2, 3, N)), rng.standard_normal((2, N)), rng.standard_normal((2, 3, NB))
    bank_v[0, 2, 0] = 0.0                # a signed zero must come out as torch makes it
    v, p, b = rng.standard_normal((3, 3, N)), rng.standard_normal((3, N)), rng.standard_normal((3, 3, NB))
    for flip, shift in itertools.product((0, 1), range(nz)):
        ov, op, ob = restore_ref(blocks, 3, nz, v, p, b, bank_v, bank_p, bank_b, [(1, 1, flip, shift)])
        for e in (0, 2):
            assert np.array_equal(_bits(ov[e]), _bits(v[e])) and np.array_equal(_bits(op[e]), _bits(p[e])) and np.array_equal(_bits(ob[e]), _bits(b[e]))

        def way(t, signed):             # [C, nz, ...]: the torch sequence
            t = torch.from_numpy(t.copy())
            if flip:
                t = torch.flip(t, dims=[1])
                if signed:
                    t[2] = -t[2]
            return torch.roll(t, shifts=shift, dims=1).numpy()

        for blk in blocks:
            nx, ny, _ = blk.size
            cells = slice(blk.cell_offset, blk.cell_offset + nx * ny * nz)
            assert np.array_equal(_bits(ov[1][:, cells]), _bits(way(bank_v[1][:, cells].reshape(3, nz, ny, nx), True).reshape(3, -1))), (flip, shift)
            assert np.array_equal(_bits(op[1][cells]), _bits(way(bank_p[1][None, cells].reshape(1, nz, ny, nx), False).reshape(-1)))
            for f, length in ((0, ny), (3, nx)):
                s0 = blk.boundary_slot0[f]
                face = way(bank_b[1][:, s0:s0 + nz * length].reshape(3, nz, length), True).reshape(3, -1)
                assert np.array_equal(_bits(ob[1][:, s0:s0 + nz * length]), _bits(face))
    # without a span symmetry (nz None) every segment is one plane and the record a copy
    ov, op, ob = restore_ref(blocks, 3, None, v, p, b, bank_v, bank_p, bank_b, [(2, 0, 0, 0)])
    assert np.array_equal(_bits(ov[2]), _bits(bank_v[0])) and np.array_equal(_bits(op[2]), _bits(bank_p[0])) and np.array_equal(_bits(ob[2]), _bits(bank_b[0]))


def test_span_symmetry():
    from fluidgym_amd.envs.airfoil_grid import make_airfoil_mesh
    from fluidgym_amd.envs.cylinder_grid import extrude_mesh, make_vortex_street_mesh

    m2 = make_vortex_street_mesh(4)
    m3 = extrude_mesh(m2, 3)
    every = [True] * len(m3.coords)
    assert all(c.dtype == np.float32 for c in m3.coords)
    assert span_symmetry(m3.coords, every) == 3
    assert span_symmetry([c.astype(np.float64) for c in m3.coords], every) == 3          # a float32 mesh held in doubles
    a2 = make_airfoil_mesh(resolution_div=4, attack_angle_deg=10.0)
    a3 = extrude_mesh(a2, 96, -0.7, 0.7)
    assert span_symmetry(a3.coords, [True] * len(a3.coords)) == 96
    # one z layer moved by 1e-3 of its spacing
    moved = [c.copy() for c in m3.coords]
    for c in moved:
        c[2, 1] += np.float32(1e-3 * 4.0 / 3.0)
    assert span_symmetry(moved, every) is None
    # a mesh with one block not z-periodic; any 2-D mesh; x not the same in every layer
    assert span_symmetry(m3.coords, [True] * (len(m3.coords) - 1) + [False]) is None
    assert span_symmetry(m2.coords, [True] * len(m2.coords)) is None
    assert span_symmetry(a2.coords, [False] * len(a2.coords)) is None
    sheared = [c.copy() for c in m3.coords]
    sheared[0][0, 2] += np.float32(1e-6)
    assert span_symmetry(sheared, every) is None
    # equal spacing in doubles is held to doubles
    z = np.linspace(0.0, 0.9, 4)
    prism = lambda zz: [np.ascontiguousarray(np.concatenate([np.broadcast_to(m2.coords[0].astype(np.float64)[:, None] + 1e-9, (2, 4) + m2.coords[0].shape[1:]),
                                                             np.broadcast_to(zz[None, :, None, None], (1, 4) + m2.coords[0].shape[1:])]))]
    assert span_symmetry(prism(z), [True]) == 3
    assert span_symmetry(prism(z + np.array([0, 1e-9, 0, 0])), [True]) is None


def test_mesh_state_bank_from_cpu_tensors():
    mk = lambda nb, k: {"velocity": torch.full((nb, 2, 7), float(k)), "pressure": torch.full((nb, 7), float(k)),
                        "boundary_velocity": torch.full((nb, 2, 5), float(k)), "solver_hints": torch.zeros(48, dtype=torch.int32)}
    snaps = [mk(2, 0), {"domain": mk(2, 1), "n_steps": 3}]
    for s in snaps:
        s.get("domain", s)["velocity"][1] += 0.5
    bank = MeshStateBank(snaps)                   # every env of every snapshot
    assert len(bank) == 4 and bank.fields["velocity"][:, 0, 0].tolist() == [0.0, 0.5, 1.0, 1.5]
    assert sorted(bank.fields) == ["boundary_velocity", "pressure", "velocity"] and bank.fields["boundary_velocity"].shape == (4, 2, 5)
    bank = MeshStateBank(snaps, env=1)            # env 1 of each
    assert bank.size == 2 and bank.fields["velocity"][:, 0, 0].tolist() == [0.5, 1.5]
    assert all(t.is_contiguous() for t in bank.fields.values())
    with pytest.raises(ValueError):
        MeshStateBank([])
    with pytest.raises(ValueError):
        MeshStateBank([mk(1, 0), {k: v for k, v in mk(1, 0).items() if k != "pressure"}])
    other = mk(1, 0)
    other["pressure"] = torch.zeros(1, 8)
    with pytest.raises(ValueError):
        MeshStateBank([mk(1, 0), other])
    with pytest.raises(ValueError):
        MeshStateBank([mk(2, 0)], env=2)


def test_parallel_env_stubs_refuse():
    from fluidgym_amd.envs.parallel_env import ParallelFluidEnv

    env = object.__new__(ParallelFluidEnv)
    for name, args in (("reset_mesh_envs", ([0],)), ("set_mesh_state_bank", ([],)), ("record_mesh_state_bank", (3,))):
        with pytest.raises(NotImplementedError, match=f"{name} is not implemented for ParallelFluidEnv"):
            getattr(env, name)(*args)
