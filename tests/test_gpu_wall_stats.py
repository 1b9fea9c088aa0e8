"""``fg_mb_wall_distribution`` / ``fg_mb_wall_moments`` on the GPU, both libraries, on synthetic flat fields and made-up ring tables
(no env): the faces against the NumPy twin in the same dtype, independence of a face from the launch, the batch around it, the
pointer alignment and the viscosity form, what a non-finite cell and an index outside the field do, the merged moments against
``HostWallMoments`` fed with the GPU's own distributions, and the argument checks.

Shapes ``(n, layers, batch)``: the ring wrap at n = 1 and n = 3, a ring that is no multiple of a wave, and more than one workgroup of
256 threads."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from fluidgym_amd import _lib as L
from fluidgym_amd.simulation.wall_stats import HostWallMoments, WallMoments, sample_wall_faces
from tests.wall_stats_ref import BOUND_TWINS, FACE_ULPS, bad_argument_lists, make_fields, make_ring

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (3, 1, 2), (67, 3, 2), (300, 2, 3)]
DTYPES = {"fp32": (np.float32, torch.float32), "fp64": (np.float64, torch.float64)}
CASES = [(shape, lib) for shape in SHAPES for lib in DTYPES]
NU = 0.013


def _setup(shape, lib, seed=0, sample=0):
    """Host fields and tables of a case: dims = 2 on one layer, 3 otherwise (the spanwise component is never read)."""
    n, layers, B = shape
    npd = DTYPES[lib][0]
    ci, si, geom, N, NB = make_ring(n, layers, seed=seed + n, dtype=npd)
    u, ub, p = make_fields(B, 2 if layers == 1 else 3, N, NB, seed=seed + n, dtype=npd, sample=sample)
    return (u, ub, p), (ci, si, geom)


def _dev(fields, tables, shift=0):
    """Everything on the device; ``shift``: the fields moved by that many elements inside a larger allocation."""
    out = []
    for a in fields:
        t = torch.as_tensor(a).cuda()
        if shift:
            buf = torch.empty(t.numel() + shift, dtype=t.dtype, device="cuda")
            buf[shift:].copy_(t.reshape(-1))
            t = buf[shift:].view(t.shape)
            assert t.data_ptr() % 16 and t.is_contiguous()
        out.append(t)
    return out, [torch.as_tensor(a).cuda().contiguous() for a in tables]


def _lib(t):
    return L.load_f64() if t.dtype == torch.float64 else L.load()


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _distribution(fields, tables, nu=NU, nu_B=None):
    """One launch of fg_mb_wall_distribution on device tensors -> out [B, 4, layers, n] (device)."""
    (u, ub, p), (ci, si, geom) = fields, tables
    B, d, N = u.shape
    layers, n = ci.shape
    out = torch.full((B, 4, layers, n), 7.0, dtype=u.dtype, device="cuda")
    so = _lib(u)
    L.check(so.fg_mb_wall_distribution(_ptr(u), _ptr(ub), _ptr(p), d, B, N, ub.shape[2], _ptr(ci), _ptr(si), _ptr(geom), n, layers, nu,
                                       _ptr(nu_B), _ptr(out), None), lib=so)
    torch.cuda.synchronize()
    return out


def _moments(samples, tables, span_average, env=None, garbage=False):
    """A WallMoments fed with ``samples`` (lists of device fields); ``env``: that env alone; ``garbage``: the accumulators hold
    NaN and huge numbers before the first sample."""
    B = samples[0][0].shape[0] if env is None else 1
    acc = WallMoments(*tables, B, span_average)
    if garbage:
        acc._dev = (torch.full((B, 4, acc.R), float("nan"), dtype=torch.float64, device="cuda"),
                    torch.full((B, 10, acc.R), 1e300, dtype=torch.float64, device="cuda"))
    for u, ub, p in samples:
        if env is not None:
            u, ub, p = u[env:env + 1], ub[env:env + 1], p[env:env + 1]
        acc.update(SimpleNamespace(velocity=u, boundary_velocity=ub, pressure=p), NU)
    torch.cuda.synchronize()
    return acc


@pytest.mark.parametrize("shape,lib", CASES)
def test_faces_equal_the_twin_and_do_not_depend_on_the_launch(shape, lib):
    n, layers, B = shape
    host, tabs = _setup(shape, lib)
    fields, tables = _dev(host, tabs)
    got = _distribution(fields, tables)
    want, scale = sample_wall_faces(*host, *tabs, NU, DTYPES[lib][0], with_scale=True)
    g = got.cpu().numpy()
    assert g.shape == want.shape == (B, 4, layers, n) and g.dtype == want.dtype
    err = np.abs(g.astype(np.float64) - want.astype(np.float64))
    bound = FACE_ULPS * np.finfo(DTYPES[lib][0]).eps * scale
    print(f"{shape} {lib}: worst face error / (eps x sum of absolute terms): {float((err / (np.finfo(DTYPES[lib][0]).eps * scale)).max()):.3f}; "
          f"bit-equal to the twin: {bool(np.array_equal(g, want))}")
    assert np.all(err <= bound) and np.array_equal(g[:, 0], want[:, 0])
    # a second run; every env alone; the envs in another order; the same fields behind pointers one element further
    assert torch.equal(_distribution(fields, tables), got)
    for b in range(B):
        assert torch.equal(_distribution([t[b:b + 1] for t in fields], tables)[0], got[b])
    perm = list(range(B))[::-1]
    assert torch.equal(_distribution([t[perm].contiguous() for t in fields], tables), got[perm])
    shifted, _ = _dev(host, tabs, shift=1)
    assert torch.equal(_distribution(shifted, tables), got)
    # one viscosity per env is the scalar launch of that env
    nus = [NU * (1 + b) for b in range(B)]
    nu_B = torch.tensor(nus, dtype=DTYPES[lib][1], device="cuda")
    per_env = _distribution(fields, tables, nu=0.0, nu_B=nu_B)
    for b in range(B):
        scalar = float(nu_B[b].item())          # the value as the library's real holds it
        assert torch.equal(_distribution([t[b:b + 1] for t in fields], tables, nu=scalar)[0], per_env[b])


@pytest.mark.parametrize("lib", list(DTYPES))
def test_a_non_finite_cell_reaches_its_own_faces_only(lib):
    shape = (67, 3, 2)
    host, tabs = _setup(shape, lib)
    ci = tabs[0]
    layer, j, b = 1, 66, 1                                    # the last face of a layer: its "left" neighbour wraps to face 0
    cell = int(ci[layer, j])
    fields, tables = _dev(host, tabs)
    clean = _distribution(fields, tables)
    fields[0][b, 0, cell] = float("nan")
    dirty = _distribution(fields, tables).cpu().numpy()
    touched = np.zeros(dirty.shape, bool)
    touched[b, 1:, layer, [65, 66, 0]] = True                 # faces whose c, cl or cr is the cell; the pressure channel reads p only
    assert np.isnan(dirty[b, 1:, layer, 66]).all() and np.isnan(dirty[b, 1:, layer, 65]).all() and np.isnan(dirty[b, 1:, layer, 0]).all()
    assert np.array_equal(dirty[~touched], clean.cpu().numpy()[~touched])
    fields[2][b, cell] = float("inf")                         # the pressure of that cell: its own face, channels p, fx, fy
    both = _distribution(fields, tables).cpu().numpy()
    assert np.isinf(both[b, 0, layer, 66]) and np.array_equal(both[b, 0].ravel()[np.arange(201) != layer * 67 + 66],
                                                              clean.cpu().numpy()[b, 0].ravel()[np.arange(201) != layer * 67 + 66])
    assert np.array_equal(both[1 - b], clean.cpu().numpy()[1 - b])


@pytest.mark.parametrize("lib", list(DTYPES))
def test_an_index_outside_its_field_is_not_read(lib):
    """One past the end and -1: the faces that would read them are NaN, every other face is untouched."""
    shape = (67, 3, 2)
    host, tabs = _setup(shape, lib)
    fields, tables = _dev(host, tabs)
    clean = _distribution(fields, tables).cpu().numpy()
    ci, si = tabs[0].copy(), tabs[1].copy()
    ci[0, 10], si[2, 40] = fields[0].shape[2], -1
    got = _distribution(fields, [torch.as_tensor(ci).cuda(), torch.as_tensor(si).cuda(), tables[2]]).cpu().numpy()
    bad = np.zeros(got.shape, bool)
    bad[:, :, 0, 9:12] = True
    bad[:, :, 2, 40] = True
    assert np.isnan(got[bad]).all() and np.array_equal(got[~bad], clean[~bad])


@pytest.mark.parametrize("shape,lib", [c for c in CASES if c[0][1] == 1])
def test_first_sample_on_one_layer_stores_the_distribution(shape, lib):
    """samples = 0 on accumulators full of garbage: the mean is the distribution widened to fp64, the central sums are 0."""
    host, tabs = _setup(shape, lib)
    fields, tables = _dev(host, tabs)
    for span_average in (True, False):
        acc = _moments([fields], tables, span_average, garbage=True)
        mean, cen = acc._state()
        assert acc.samples == 1 and mean.tobytes() == _distribution(fields, tables)[:, :, 0].double().cpu().numpy().tobytes()
        assert cen.shape == (shape[2], 10, shape[0]) and not cen.any()


@pytest.mark.parametrize("span_average", [True, False], ids=["span", "faces"])
@pytest.mark.parametrize("shape,lib", CASES)
def test_four_merged_samples_equal_the_host_twin(shape, lib, span_average):
    n, layers, B = shape
    tabs = _setup(shape, lib)[1]
    hosts = [_setup(shape, lib, sample=s)[0] for s in range(4)]
    samples = [_dev(h, tabs)[0] for h in hosts]
    tables = _dev(hosts[0], tabs)[1]
    acc = _moments(samples, tables, span_average, garbage=True)
    ref = HostWallMoments(n, layers, span_average)
    dists = [_distribution(f, tables).cpu().numpy() for f in samples]
    for d in dists:
        ref.update(d)
    assert acc.samples == ref.samples == 4 and acc.count == ref.count
    (gm, gc), (hm, hc) = acc._state(), ref._state()
    # the absolute-monomial sums of the record, from the GPU's own distributions
    v = np.stack(dists).astype(np.float64)                                          # [S, B, 4, layers, n]
    c = np.moveaxis(v, 3, 1).reshape(4 * layers, B, 4, n) if span_average else v.reshape(4, B, 4, layers * n)
    dev = c - c.mean(axis=0)
    abs1 = np.abs(c).sum(axis=0) / c.shape[0]
    absM = np.stack([np.abs(dev[:, :, i] * dev[:, :, j]).sum(axis=0) for i, j in ref.pairs], axis=1)
    em = float((np.abs(gm - hm) / np.where(abs1 > 0, abs1, 1)).max())
    ec = float((np.abs(gc - hc) / np.where(absM > 0, absM, 1)).max())
    print(f"{shape} {lib} span_average={span_average}: mean {em:.2e}, central {ec:.2e} of the absolute-monomial sum; "
          f"bit-equal: {gm.tobytes() == hm.tobytes() and gc.tobytes() == hc.tobytes()}")
    assert em <= BOUND_TWINS and ec <= BOUND_TWINS
    assert np.array_equal(gc[absM == 0], hc[absM == 0])
    # accessors read the device state
    assert acc.mean("tau_w").shape == ((B, n) if span_average or layers == 1 else (B, layers, n))
    # a second run, and every env alone, repeat bit for bit
    bits = [a.tobytes() for a in acc._state()]
    assert [a.tobytes() for a in _moments(samples, tables, span_average)._state()] == bits
    for b in range(B):
        alone = _moments(samples, tables, span_average, env=b)._state()
        assert alone[0].tobytes() == gm[b:b + 1].tobytes() and alone[1].tobytes() == gc[b:b + 1].tobytes()


def test_every_invalid_argument_returns_the_code():
    for so in (L.load(), L.load_f64()):
        for name, moments in (("fg_mb_wall_distribution", False), ("fg_mb_wall_moments", True)):
            for args in bad_argument_lists(moments):
                assert getattr(so, name)(*args, None) == -1, (name, args)          # FG_ERR_INVALID_ARG
                assert name.encode() in so.fg_last_error()
    # the Python layer refuses host arrays and a batch the accumulator was not made for
    host, tabs = _setup((3, 1, 2), "fp32")
    fields, tables = _dev(host, tabs)
    acc = WallMoments(*tables, 3)
    with pytest.raises(ValueError, match="3 envs"):
        acc.update(SimpleNamespace(velocity=fields[0], boundary_velocity=fields[1], pressure=fields[2]), NU)
    with pytest.raises(ValueError, match="GPU"):
        WallMoments(*tables, 2).update(SimpleNamespace(velocity=torch.as_tensor(host[0]), boundary_velocity=torch.as_tensor(host[1]),
                                                       pressure=torch.as_tensor(host[2])), NU)
