"""``fg_plane_spectra`` / ``PlaneSpectra`` on the GPU, both libraries: three samples summed on the device against the fp64 NumPy
evaluation of the same (rounded) inputs and against the host twin, within the derived FFT error bound (``tests/plane_spectra_ref.py``);
independence of a slab from the rest of the batch and from how its rows are loaded, repeatability, what a non-finite cell does, and
the extents the kernel refuses.

Shapes ``(B, nz, ny, nx)``: the smallest extents; nz > nx; the golden shape; more columns than a wave has lanes with the mixed
radix 4 4 4 2; the largest registered plane (the LDS limit in fp64); 2-D fields, short and at the longest row."""
import ctypes
import os

import numpy as np
import pytest
import torch

from fluidgym_amd import _lib as L
from fluidgym_amd.simulation.plane_spectra import HostPlaneSpectra, PlaneSpectra
from tests.plane_spectra_ref import BOUND_GOLDEN, bound_ratios, channel_stack, direct_sums, make_samples

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_plane_spectra.npz")
SHAPES_3D = [(2, 4, 5, 8), (1, 16, 4, 8), (2, 8, 6, 16), (1, 64, 4, 128), (1, 128, 3, 128)]
SHAPES_2D = [(2, 1, 5, 32), (1, 1, 4, 512)]
CHANNELS = {3: ("u", "v", "p"), 4: ("u", "v", "w", "p"), 5: ("u", "v", "w", "p", "T")}
DTYPES = {"fp32": (np.float32, torch.float32), "fp64": (np.float64, torch.float64)}


def _planes(ny):
    return (ny - 1, 1, 0)          # unsorted, rows 0 and ny - 1 a mirror pair (listed by hand: symmetric=False below)


def _dev(sample):
    return tuple(None if f is None else torch.as_tensor(f).cuda() for f in sample)


def _gpu(samples, K, planes, symmetric=False, env=None):
    acc = PlaneSpectra(CHANNELS[K], planes, symmetric)
    for s in samples:
        f = _dev(s)
        if env is not None:
            f = tuple(None if t is None else t[env:env + 1] for t in f)      # views into the batch: the same memory, one env
        acc.update(*f)
    torch.cuda.synchronize()
    return acc


def _direct(samples, K, planes, lib, shift):
    """The entry called with every channel a contiguous tensor of its own (batch stride nz ny nx), ``shift`` reals past a 256-byte
    boundary: 0 keeps the 16-byte loads, 1 forces the scalar ones.  Returns the bytes of amp and power."""
    _, t_t = DTYPES[lib]
    B, nz, ny, nx = samples[0][1].shape[0], *((1,) + samples[0][1].shape[2:])[-3:]
    cells = nz * ny * nx
    so = L.load_f64() if lib == "fp64" else L.load()
    out = torch.zeros(2, B, K, len(planes), max(nz // 2, 1), nx // 2, dtype=torch.float64, device="cuda")
    for s in samples:
        fields = [channel for channel in channel_stack(s, K)]                # K x [B, nz, ny, nx], values exact in the dtype
        bufs = [torch.zeros(B * cells + 64, dtype=t_t, device="cuda") for _ in fields]
        for buf, f in zip(bufs, fields):
            buf[shift:shift + B * cells] = torch.as_tensor(f.reshape(-1)).to(t_t).cuda()
        ptrs = (ctypes.c_void_p * K)(*[buf.data_ptr() + shift * buf.element_size() for buf in bufs])
        strides = (ctypes.c_int64 * K)(*([cells] * K))
        rows = (ctypes.c_int32 * len(planes))(*planes)
        L.check(so.fg_plane_spectra(ptrs, strides, K, B, nz, ny, nx, rows, len(planes), ctypes.c_void_p(out[0].data_ptr()),
                                    ctypes.c_void_p(out[1].data_ptr()), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), lib=so)
        torch.cuda.synchronize()
    return [out[0].cpu().numpy().tobytes(), out[1].cpu().numpy().tobytes()]


def _bits(acc):
    return [a.tobytes() for a in acc._state()]


@pytest.mark.parametrize("lib", list(DTYPES))
@pytest.mark.parametrize("shape", SHAPES_3D + SHAPES_2D, ids=lambda s: "x".join(map(str, s)))
def test_three_summed_samples_within_the_fft_bound_of_numpy_and_the_host_twin(shape, lib):
    np_t, _ = DTYPES[lib]
    eps = float(np.finfo(np_t).eps)
    B, nz, ny, nx = shape
    for K in ((3,) if shape in SHAPES_2D else (4, 5)):
        samples = make_samples(shape, K, seed=sum(shape) + K, dtype=np_t)
        truth = direct_sums([channel_stack(s, K) for s in samples], list(_planes(ny)))
        acc = _gpu(samples, K, _planes(ny))
        count, amp, power = acc._state()
        ra, rp = bound_ratios(amp, power, truth, eps, nz, nx)
        host = HostPlaneSpectra(CHANNELS[K], _planes(ny), False)
        for s in samples:
            host.update(*s)
        ha, hp = bound_ratios(amp, power, host._state()[1:] + truth[2:], eps, nz, nx)
        print(f"{shape} {lib} K {K}: error / bound against numpy amp {ra:.3g} power {rp:.3g}; against the host twin amp {ha:.3g} power {hp:.3g}")
        assert ra <= 1 and rp <= 1 and ha <= 1 and hp <= 1
        assert count.tolist() == [3.0] * B and acc.samples == 3 and acc.n == 3 * B
        assert amp.shape == (B, K, 3, max(nz // 2, 1), nx // 2) and np.all(power >= 0)


def test_the_golden_shape_against_the_reference_values():
    g = np.load(GOLDEN)
    acc = PlaneSpectra(("u", "v", "w"), (0, 2), True)
    for s in range(3):
        acc.update(torch.as_tensor(g["velocity"][s]).cuda())
    assert acc.n == int(g["n"])
    # the device transform is no pocket FFT: the derived bound, per element from the slabs that enter it (all below the largest)
    lg = np.log2(8 * 16)
    worst_norm = max(np.sqrt((np.abs(np.fft.fftn(g["velocity"][s][:, :, :, [0, 2, 5, 3]], axes=(2, 4))) ** 2).sum(axis=(2, 4))).max() for s in range(3))
    err = float(np.abs(acc.reference_fft() - g["fft"]).max())
    print(f"golden fft: worst error {err:.3e}, bound {8 * np.finfo(np.float64).eps * lg * worst_norm:.3e}, "
          f"{err / g['fft'].max():.2e} of the largest amplitude (host twin: {BOUND_GOLDEN:.0e})")
    assert err <= 8 * np.finfo(np.float64).eps * lg * worst_norm


@pytest.mark.parametrize("lib", list(DTYPES))
@pytest.mark.parametrize("shape,K", [((2, 4, 5, 8), 4), ((2, 8, 6, 16), 5), ((2, 64, 4, 128), 4), ((2, 1, 5, 32), 3)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_slabs_are_independent_repeatable_and_a_nan_stays_in_its_slab(shape, K, lib):
    np_t, _ = DTYPES[lib]
    B, nz, ny, nx = shape
    planes = _planes(ny)
    samples = make_samples(shape, K, seed=17, dtype=np_t)
    full = _gpu(samples, K, planes)
    assert _bits(full) == _bits(_gpu(samples, K, planes))                     # fresh accumulators, same bits
    _, amp, power = full._state()
    for b in range(B):                                                        # env b of the batch = env b alone
        _, ba, bp = _gpu(samples, K, planes, env=b)._state()
        assert ba.tobytes() == amp[b:b + 1].tobytes() and bp.tobytes() == power[b:b + 1].tobytes()
    for shift in (0, 1):                                                      # slices in place = contiguous copies, however they are loaded
        assert _direct(samples, K, planes, lib, shift) == _bits(full)[1:]
    where = (B - 1, 1, ny - 1, nx - 1) if nz == 1 else (B - 1, 1, nz - 1, ny - 1, nx - 1)      # sample 1, channel v, row ny - 1
    samples[1][0][where] = np.nan
    _, da, dp = _gpu(samples, K, planes)._state()
    bad = np.zeros((B, K, 3), bool)
    bad[B - 1, 1, 0] = True
    for clean, dirty in ((amp, da), (power, dp)):
        assert np.isnan(dirty[bad]).all() and clean[~bad].tobytes() == dirty[~bad].tobytes()


def test_merge_pooled_and_a_changed_shape():
    samples = make_samples((2, 8, 6, 16), 4, seed=23)
    a, b = _gpu(samples[:2], 4, (1, 4), True), _gpu(samples[2:], 4, (1, 4), True)
    whole = _gpu(samples, 4, (1, 4), True)
    a.merge(b)
    assert a.samples == 3 and a.n == whole.n == 12
    for x, y in zip(a._state(), whole._state()):
        assert np.allclose(x, y, rtol=1e-14, atol=0)
    a.update(*_dev(samples[0]))                                               # the merged state is the device state
    assert a.n == 16 and a.pooled().amplitude("p").shape == (1, 2, 4, 8)
    with pytest.raises(ValueError, match="changed between updates"):
        a.update(*_dev(make_samples((3, 8, 6, 16), 4)[0]))


@pytest.mark.parametrize("lib", list(DTYPES))
def test_unsupported_extents_raise_before_anything_is_launched(lib):
    _, t_t = DTYPES[lib]
    cases = [(8, 24), (8, 1024), (2, 16)] + ([(256, 128)] if lib == "fp64" else [(256, 512)])
    for nz, nx in cases:
        u = torch.zeros(1, 3, nz, 2, nx, dtype=t_t, device="cuda")
        p = torch.zeros(1, 1, nz, 2, nx, dtype=t_t, device="cuda")
        acc = PlaneSpectra(planes=(0,))
        with pytest.raises(ValueError, match="power of two|LDS"):
            acc.update(u, p)
        assert acc._dev is None and acc.samples == 0                          # nothing allocated, nothing counted
        # the direct call answers FG_ERR_UNSUPPORTED and leaves the accumulators alone
        lib_ = L.load_f64() if lib == "fp64" else L.load()
        out = torch.full((2, 4, 2, max(nz // 2, 1), nx // 2), 7.0, dtype=torch.float64, device="cuda")
        cells = nz * 2 * nx
        ptrs = (ctypes.c_void_p * 4)(*([u.data_ptr() + c * cells * u.element_size() for c in range(3)] + [p.data_ptr()]))
        strides = (ctypes.c_int64 * 4)(3 * cells, 3 * cells, 3 * cells, cells)
        rows = (ctypes.c_int32 * 2)(0, 1)
        rc = lib_.fg_plane_spectra(ptrs, strides, 4, 1, nz, 2, nx, rows, 2, ctypes.c_void_p(out[0].data_ptr()), ctypes.c_void_p(out[1].data_ptr()),
                                   ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert rc == L.FG_ERR_UNSUPPORTED and bool((out == 7.0).all())
