"""``MultiBlockDomain.RestoreEnvs`` (``fg_mb_restore_envs``) on the GPU, fp32 and fp64: the copy and the span
transform bit for bit against the NumPy restatement, the reset noise bit for bit against ``tests/obs_noise_ref.py`` and independent
of the batch, nothing stale after a restore, the map as a symmetry of the solver, and the refusals."""
import itertools

import numpy as np
import pytest
import torch

from fluidgym_amd.simulation.mb_state_bank import MeshStateBank
from tests import helpers_mb as H
from tests.mb_env_restore_ref import restore_ref, source_index

pytestmark = pytest.mark.gpu

DTYPES = {"fp32": (torch.float32, np.float32), "fp64": (torch.float64, np.float64)}
MESHES = {"odd_channel": H.odd_channel, "cylinder_2d": lambda: H.cylinder_2d(8), "skewed_pair_3d": lambda: H.skewed_pair_3d(nz=3),
          "cylinder_3d_small": lambda: H.cylinder_3d_small(4, 3)}
FIELDS = ("velocity", "pressure", "boundary_velocity")


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _fill(dom, npt, seed):
    """Distinct random values in the three arrays of every env; returns them as host arrays."""
    rng = np.random.default_rng(seed)
    host = {}
    for k in FIELDS:
        t = getattr(dom, k)
        host[k] = rng.standard_normal(tuple(t.shape)).astype(npt)
        t.copy_(torch.from_numpy(host[k]))
    return host


def _bank(dom, npt, S, seed):
    rng = np.random.default_rng(seed)
    host = {k: rng.standard_normal((S,) + tuple(getattr(dom, k).shape[1:])).astype(npt) for k in FIELDS}
    return MeshStateBank([{k: torch.from_numpy(v).to(dom.device) for k, v in host.items()}]), host


def _ref(dom, before, bank_host, records, noise=None):
    return restore_ref(dom.blocks, dom.dims, dom.span_nz(), before["velocity"], before["pressure"], before["boundary_velocity"],
                       bank_host["velocity"], bank_host["pressure"], bank_host["boundary_velocity"], records, noise)


def _assert_equal(dom, expected, what=""):
    for k, e in zip(FIELDS, expected):
        got = getattr(dom, k)
        bad = np.nonzero(_bits(got) != _bits(e))
        assert bad[0].size == 0, (what, k, [int(x[0]) for x in bad], bad[0].size)


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("mesh", list(MESHES))
def test_copy_and_transform_bit_for_bit(mesh, dtype):
    tdt, npt = DTYPES[dtype]
    dom = MESHES[mesh]().native(batch=6, dtype=tdt)
    try:
        before = _fill(dom, npt, 1)
        bank, bank_host = _bank(dom, npt, 2, 2)
        if dom.dims == 3:
            assert dom.span_nz() == 3
            combos = list(itertools.product((0, 1), range(3)))
            records = [(e, e % 2, f, s) for e, (f, s) in enumerate(combos)]
        else:
            assert dom.span_nz() is None
            records = [(4, 1, 0, 0), (1, 0, 0, 0)]
        envs, src, flip, shift = (list(c) for c in zip(*records))
        dom.RestoreEnvs(bank, envs, src, flip, shift)
        torch.cuda.synchronize()
        _assert_equal(dom, _ref(dom, before, bank_host, records), mesh)
        named = set(envs)
        for k in FIELDS:              # the envs that were not named keep their bits (2-D: four of six)
            for e in set(range(6)) - named:
                assert np.array_equal(_bits(getattr(dom, k)[e]), _bits(before[k][e])), (k, e)
        assert len(named) == (6 if dom.dims == 3 else 2)
    finally:
        dom.close()


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("mesh", ["odd_channel", "skewed_pair_3d"])
def test_noise_bit_for_bit_and_independent_of_the_batch(mesh, dtype):
    tdt, npt = DTYPES[dtype]
    spec = MESHES[mesh]()
    dom, small = spec.native(batch=3, dtype=tdt), spec.native(batch=2, dtype=tdt)
    try:
        seed, sv, sp = 0x123456789ABCDEF, 0.025, 0.01
        z = (1, 2) if dom.dims == 3 else (0, 0)
        bank, bank_host = _bank(dom, npt, 2, 3)
        # env 1 alone
        before = _fill(dom, npt, 4)
        dom.RestoreEnvs(bank, [1], 1, z[0], z[1], noise=(seed, sv, sp, [5]))
        _assert_equal(dom, _ref(dom, before, bank_host, [(1, 1, z[0], z[1])], (seed, sv, sp, [5])), "alone")
        alone = {k: getattr(dom, k)[1].clone() for k in FIELDS}
        # together with env 0 (another source, episode and transform)
        before = _fill(dom, npt, 5)
        dom.RestoreEnvs(bank, [0, 1], [0, 1], [0, z[0]], [0, z[1]], noise=(seed, sv, sp, [2, 5]))
        _assert_equal(dom, _ref(dom, before, bank_host, [(0, 0, 0, 0), (1, 1, z[0], z[1])], (seed, sv, sp, [2, 5])), "pair")
        for k in FIELDS:
            assert np.array_equal(_bits(getattr(dom, k)[1]), _bits(alone[k])), k
        assert not torch.equal(dom.velocity[0], dom.velocity[1])
        # in a domain of another batch size
        _fill(small, npt, 6)
        small.RestoreEnvs(bank, [1], 1, z[0], z[1], noise=(seed, sv, sp, [5]))
        for k in FIELDS:
            assert np.array_equal(_bits(getattr(small, k)[1]), _bits(alone[k])), k
        # another episode: another field
        small.RestoreEnvs(bank, [1], 1, z[0], z[1], noise=(seed, sv, sp, [6]))
        assert not torch.equal(small.velocity[1], alone["velocity"]) and not torch.equal(small.pressure[1], alone["pressure"])
        assert np.array_equal(_bits(small.boundary_velocity[1]), _bits(alone["boundary_velocity"]))       # boundary values get no noise
        # noise=None: the pure copy, and the boundary array of the noisy restore is the pure copy's
        before = _fill(small, npt, 7)
        small.RestoreEnvs(bank, [1], 1, z[0], z[1], noise=None)
        _assert_equal(small, _ref(small, before, bank_host, [(1, 1, z[0], z[1])]), "copy")
        assert np.array_equal(_bits(small.boundary_velocity[1]), _bits(alone["boundary_velocity"]))
        # sigma 0 runs the same arithmetic and adds a zero
        small.RestoreEnvs(bank, [1], 1, z[0], z[1], noise=(seed, 0.0, 0.0, [5]))
        assert torch.equal(small.velocity[1], torch.from_numpy(_ref(small, before, bank_host, [(1, 1, z[0], z[1])])[0][1]).to(small.device))
    finally:
        dom.close()
        small.close()


def test_nothing_stale_after_a_restore():
    """Two sim steps, a restore of env 1, one PISO step -- against a fresh domain brought to the same three arrays by ``copy_``: the
    three bound arrays are all a handle carries between steps."""
    spec = H.cylinder_2d(8)
    dom, fresh = spec.native(batch=3), spec.native(batch=3)
    try:
        dom.single_step(0.02)
        donor = {k: getattr(dom, k)[0:1].clone() for k in FIELDS}
        dom.single_step(0.02)
        dom.RestoreEnvs(MeshStateBank([donor]), [1])
        assert torch.equal(dom.velocity[1], donor["velocity"][0]) and not torch.equal(dom.velocity[0], donor["velocity"][0])
        for k in FIELDS:
            getattr(fresh, k).copy_(getattr(dom, k))
        fresh.solver_hints(dom.solver_hints().tolist())
        dom.piso_step(0.01)
        fresh.piso_step(0.01)
        assert np.array_equal(_bits(dom.velocity[1]), _bits(fresh.velocity[1]))
        assert np.array_equal(_bits(dom.pressure[1]), _bits(fresh.pressure[1]))
        assert torch.isfinite(dom.velocity).all() and not torch.equal(dom.velocity[1], donor["velocity"][0])
    finally:
        dom.close()
        fresh.close()


TIGHT = dict(advection_tol=1e-13, pressure_tol=1e-13, max_iterations=20000, raise_on_failure=False)


def test_the_map_is_a_symmetry_of_the_solver():
    """fp64, the skewed two-block prism: ``piso_step(T s)`` against ``T(piso_step(s))`` for every mirror and roll, ``T`` applied by
    ``RestoreEnvs`` from a one-state bank.  Bound ``2e-9 max|u|``: tests/test_gpu_mb_f64.py states 1e-9 for a whole step at these
    tolerances, and two computed steps are compared.  A transform that forgets the sign of ``w`` must miss the bound."""
    nz, dt = 3, 0.02
    dom = H.skewed_pair_3d(nz=nz).native(batch=1, dtype=torch.float64)
    try:
        assert dom.span_nz() == nz
        # a z-varying tangential part on the lid, zero in the mean over z of every column: no net flux through the face
        wave = torch.tensor([np.cos(2 * np.pi * k / nz) + 0.5 * np.sin(2 * np.pi * k / nz) for k in range(nz)], dtype=torch.float64, device=dom.device)
        wave = wave - wave.mean()
        for blk in dom.blocks:
            lid = blk.boundary(3)                                    # [1, 3, nz * nx], z slowest
            v = lid.reshape(1, 3, nz, -1)
            v[:, 0] += 0.4 * wave[None, :, None]
            v[:, 2] += 0.3 * wave.roll(1)[None, :, None]
        for _ in range(3):
            dom.piso_step(dt, **TIGHT)
        s = {k: getattr(dom, k).clone() for k in FIELDS}
        dom.piso_step(dt, **TIGHT)
        stepped = {k: getattr(dom, k).clone() for k in FIELDS}
        assert float(stepped["velocity"][0, 2].abs().max()) > 1e-2      # w takes part
        bank_s, bank_stepped = MeshStateBank([s]), MeshStateBank([stepped])
        scale = float(stepped["velocity"].abs().max())
        bound = 2e-9 * scale
        for flip, shift in itertools.product((0, 1), range(nz)):
            dom.RestoreEnvs(bank_s, [0], 0, flip, shift)
            dom.piso_step(dt, **TIGHT)
            first = dom.velocity.clone()
            dom.RestoreEnvs(bank_stepped, [0], 0, flip, shift)
            err = float((first - dom.velocity).abs().max())
            print(f"flip_z={flip} shift_z={shift}: max|piso(T s) - T piso(s)| = {err:.3e} (bound {bound:.3e})")
            assert err <= bound, (flip, shift, err, bound)
        # the mirror without the sign of w, formed with torch: a permutation that is no symmetry
        cell, slot = source_index(dom.blocks, 3, nz, dom.n_cells, dom.n_boundary_faces, 1, 0)
        cell, slot = torch.from_numpy(cell).to(dom.device), torch.from_numpy(slot).to(dom.device)
        wrong = lambda st: {"velocity": st["velocity"][..., cell], "pressure": st["pressure"][..., cell],
                            "boundary_velocity": st["boundary_velocity"][..., slot]}
        for k, t in wrong(s).items():
            getattr(dom, k).copy_(t)
        dom.piso_step(dt, **TIGHT)
        err = float((dom.velocity - wrong(stepped)["velocity"]).abs().max())
        print(f"mirror without the sign of w: {err:.3e}")
        assert err > bound, "the inputs are too symmetric: the test proves nothing"
    finally:
        dom.close()


def test_restore_envs_refuses_a_span_transform_where_there_is_no_symmetry():
    flat = H.odd_channel().native(batch=2)
    spec = H.skewed_pair_3d(nz=3)
    spec.blocks = [H.extrude(c[:2, 0], np.array([0.0, 0.2, 0.5, 0.9])) for c in spec.blocks]         # layers of unequal thickness
    uneven = spec.native(batch=2)
    try:
        for dom in (flat, uneven):
            assert dom.span_nz() is None
            bank = MeshStateBank([dom.Clone()])
            for kw in (dict(flip_z=1), dict(shift_z=1), dict(flip_z=[0, 1])):
                with pytest.raises(ValueError):
                    dom.RestoreEnvs(bank, [0, 1], 0, **kw)
            dom.RestoreEnvs(bank, [0, 1], [1, 0])                    # the copy is there for every mesh
            for bad in (dict(envs=[0, 0]), dict(envs=[2]), dict(envs=[0], src=2), dict(envs=[0], noise=(1, -0.1, 0.0, [0])),
                        dict(envs=[0], noise=(1, 0.0, float("nan"), [0]))):
                with pytest.raises(ValueError):
                    dom.RestoreEnvs(bank, **bad)
    finally:
        flat.close()
        uneven.close()
