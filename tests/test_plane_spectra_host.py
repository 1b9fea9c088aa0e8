"""Plane spectra without a GPU: ``HostPlaneSpectra`` against the reference's golden values and against a direct one-shot
``numpy.fft.fftn`` evaluation, merging, pooling, mirror planes, files, and the ABI of ``fg_plane_spectra``."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

from fluidgym_amd import _lib as L
from fluidgym_amd.simulation.plane_spectra import HostPlaneSpectra, PlaneSpectra, check_extents, lds_bytes
from tests.plane_spectra_ref import BOUND_GOLDEN, bound_ratios, channel_stack, direct_sums, make_samples

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_plane_spectra.npz")
CHANNELS = {3: ("u", "v", "p"), 4: ("u", "v", "w", "p"), 5: ("u", "v", "w", "p", "T")}
EPS = np.finfo(np.float64).eps


def _run(samples, K, planes, symmetric=True):
    acc = HostPlaneSpectra(CHANNELS[K], planes, symmetric)
    for u, p, T in samples:
        acc.update(u, p, T)
    return acc


def _golden_record(g):
    acc = HostPlaneSpectra(("u", "v", "w"), (0, 2), True)
    for s in range(3):
        acc.update(g["velocity"][s])
    return acc


def test_the_reference_golden_values():
    g = np.load(GOLDEN)
    acc = _golden_record(g)
    assert acc.samples == 3 and acc.n == int(g["n"]) == 12
    scale = float(g["fft"].max())
    fft = acc.reference_fft()
    assert fft.shape == g["fft"].shape == (3, 4, 2, 8)
    e_fft = float(np.abs(fft - g["fft"]).max()) / scale
    phys, nu, utau = g["phys_sizes"].tolist(), float(g["nu"]), float(g["utau"])
    pooled = acc.pooled()
    lam, phi = zip(*(pooled.premultiplied(c, phys, nu, utau) for c in "uvw"))
    phi = np.stack([p[0].transpose(1, 0, 2) for p in phi])                      # [1, P, nkz, nkx] per channel -> [3, nkz, P, nkx]
    e_phi = float(np.abs(phi - g["phi"]).max()) / float(g["phi"].max())
    e_lam = max(float(np.abs(lam[0][0] / g["lambda_z"] - 1).max()), float(np.abs(lam[0][1] / g["lambda_x"] - 1).max()))
    print(f"against the golden values: fft {e_fft:.2e}, phi {e_phi:.2e} of the largest value; wavelengths {e_lam:.2e} relative")
    assert e_fft <= BOUND_GOLDEN and e_phi <= BOUND_GOLDEN and e_lam <= BOUND_GOLDEN
    # per-env spectra average to the pooled one, the mirror folded in
    assert np.allclose(acc.amplitude("u").mean(axis=0), pooled.amplitude("u")[0], rtol=1e-14, atol=0)
    # the reference's k grid is the outer product only where nz == nx; both layouts hold the same factors
    assert sorted(acc.k_grid().ravel()) == sorted(acc.k_grid(reference_layout=False).ravel())
    assert np.array_equal(acc.k_grid(False), np.outer(np.arange(1, 5), np.arange(1, 9)))


@pytest.mark.parametrize("K,shape", [(4, (2, 8, 6, 16)), (5, (2, 4, 5, 8)), (3, (2, 1, 5, 32))], ids=str)
def test_merged_pooled_and_mirrored_records_equal_the_one_shot(K, shape):
    B, nz, ny, nx = shape
    samples = make_samples(shape, K, samples=4, seed=31, dtype=np.float64)
    stacks = [channel_stack(s, K) for s in samples]
    planes = (ny - 2, 0)
    acc = _run(samples, K, planes)
    table = acc.plane_table(ny)
    assert table == [ny - 2, 0, 1, ny - 1]
    truth = direct_sums(stacks, table)
    _, amp, power = acc._state()
    ra, rp = bound_ratios(amp, power, truth, EPS, nz, nx)
    print(f"{shape} K {K}: amp {ra:.3f}, power {rp:.3f} of the bound")
    assert ra <= 1 and rp <= 1 and acc.n == 2 * B * 4 and acc.samples == 4
    # two halves merged are the record of all samples
    halves = _run(samples[:1], K, planes).merge(_run(samples[1:], K, planes))
    assert halves.samples == 4 and halves.n == acc.n
    assert max(bound_ratios(*halves._state()[1:], truth, EPS, nz, nx)) <= 1
    assert np.allclose(halves.amplitude(0), acc.amplitude(0), rtol=1e-14, atol=0)
    # pooled(): one ensemble of all envs
    pooled = acc.pooled()
    t_pool = tuple(t.sum(axis=0, keepdims=True) for t in truth)
    assert max(bound_ratios(*pooled._state()[1:], t_pool, EPS, nz, nx)) <= 1.0 and pooled.n == acc.n
    assert pooled.amplitude("v").shape == (1, 2, max(nz // 2, 1), nx // 2)
    # symmetric against the mirror planes listed by hand
    listed = _run(samples, K, tuple(table), symmetric=False)
    assert listed.n == B * 4
    for ch in range(K):
        by_hand = 0.5 * (listed.amplitude(ch)[:, :2] + listed.amplitude(ch)[:, 2:])
        assert np.allclose(acc.amplitude(ch), by_hand, rtol=1e-14, atol=0)
        assert np.allclose(acc.power(ch), 0.5 * (listed.power(ch)[:, :2] + listed.power(ch)[:, 2:]), rtol=1e-14, atol=0)
    assert np.allclose(acc.power("u")[0, 1], truth[1][0, 0, [1, 3]].sum(axis=0) / 8, rtol=1e-12, atol=0)


def test_a_non_finite_cell_poisons_its_slab_only():
    samples = make_samples((2, 4, 5, 8), 4, seed=5, dtype=np.float64)
    clean = _run(samples, 4, (1, 2), symmetric=False)
    samples[1][0][1, 2, 3, 2, 4] = np.nan            # sample 1, env 1, channel w, z 3, y 2, x 4
    dirty = _run(samples, 4, (1, 2), symmetric=False)
    bad = np.zeros((2, 4, 2), bool)
    bad[1, 2, 1] = True
    for a, b in zip(clean._state()[1:], dirty._state()[1:]):
        assert np.isnan(b[bad]).all() and a[~bad].tobytes() == b[~bad].tobytes()


def test_save_load_round_trip_and_the_reference_file_layout(tmp_path):
    g = np.load(GOLDEN)
    acc = _golden_record(g)
    acc.save(tmp_path, "PSD")
    with np.load(tmp_path / "PSD.npz") as z:
        assert set(g["keys_psd"].tolist()) <= set(z.keys()) and {"amp_sum", "power_sum", "channels"} <= set(z.keys())
        assert int(z["n"]) == 12 and z["fft"].shape == (3, 4, 2, 8)
        assert np.abs(z["fft"] - g["fft"]).max() <= BOUND_GOLDEN * g["fft"].max()
    with open(tmp_path / "PSD.json") as f:
        params = json.load(f)
    assert sorted(params) == g["json_names"].tolist() and params == json.loads(str(g["json_values"]))
    back = HostPlaneSpectra.load(tmp_path, "PSD")
    for a, b in zip(acc.pooled()._state(), back._state()):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    assert (back.channels, back.planes, back.symmetric, back.samples, back.grid, back.n) == (acc.channels, acc.planes, True, 3, (8, 6, 16), 12)
    # 2-D records and records with more channels keep the reference's layout of the velocity part
    flat = _run(make_samples((2, 1, 5, 32), 3, seed=2, dtype=np.float64), 3, (1,))
    flat.save(tmp_path / "flat", "rbc")
    with np.load(tmp_path / "flat" / "rbc.npz") as z:
        assert z["fft"].shape == (2, 1, 16) and int(z["n"]) == 12
    assert flat.reference_parameters()["fft_dims"] == [3] and flat.wavelengths([2.0], 1e-3, 0.05)[0].shape == (16,)
    with pytest.raises(ValueError, match="u, v"):
        _run_p_only().save(tmp_path / "p")


def _run_p_only():
    acc = HostPlaneSpectra(("p",), (0,), False)
    acc.update(np.zeros((1, 2, 4, 8)), np.ones((1, 1, 4, 8)))
    return acc


def test_arguments_the_python_layer_refuses():
    z5 = lambda nz, nx: (np.zeros((1, 3, nz, 4, nx)), np.zeros((1, 1, nz, 4, nx)))
    for nz, nx, rule in ((8, 24, "nx must be a power of two"), (8, 1024, "nx must be a power of two"), (2, 16, "nz must be 1 or a power"),
                         (512, 16, "nz must be 1 or a power"), (6, 16, "nz must be 1 or a power"), (4, 4, "nx must be a power of two")):
        with pytest.raises(ValueError, match=rule):
            HostPlaneSpectra(planes=(0,)).update(*z5(nz, nx))
    with pytest.raises(ValueError, match="fit in 160 KB of LDS"):
        check_extents(256, 128, 8)
    check_extents(256, 128, 4)
    for nz, nx in ((64, 64), (128, 128), (64, 128), (128, 64), (1, 512)):      # every registered TCF plane, both libraries
        check_extents(nz, nx, 4)
        check_extents(nz, nx, 8)
    assert lds_bytes(128, 128, 8) == (128 + 128 * 65 + 8 * 128) * 16 + 16 and lds_bytes(64, 128, 4) == (128 + 64 * 65 + 8 * 256) * 8 + 16
    with pytest.raises(ValueError, match="planes"):
        HostPlaneSpectra(planes=())
    with pytest.raises(ValueError, match="planes"):
        HostPlaneSpectra(planes=tuple(range(17)), symmetric=True)
    with pytest.raises(ValueError, match="outside the 4 rows"):
        HostPlaneSpectra(planes=(4,)).update(*z5(4, 8))
    with pytest.raises(ValueError, match="channels"):
        HostPlaneSpectra(("u", "u"))
    with pytest.raises(ValueError, match="multi-block"):
        HostPlaneSpectra().update(np.zeros((1, 3, 40)), np.zeros((1, 1, 40)))
    with pytest.raises(ValueError, match="GPU"):
        PlaneSpectra().update(*z5(4, 8))
    acc = HostPlaneSpectra(planes=(0,))
    acc.update(*z5(4, 8))
    with pytest.raises(ValueError, match="changed between updates"):
        acc.update(*z5(4, 16))
    with pytest.raises(ValueError, match="same channels"):
        acc.merge(HostPlaneSpectra(planes=(1,)))


def test_plane_spectra_abi():
    header = open(os.path.join(ROOT, "include", "fluidgym_hip.h")).read()
    assert re.search(r"\bint\s+fg_plane_spectra\s*\(", header)
    assert "fg_plane_spectra" in L.SIGNATURES and "fg_plane_spectra" in L.SIGNATURES_F64
    assert not "fg_plane_spectra".startswith(L._F64_ABSENT_PREFIXES)
    mk = open(os.path.join(ROOT, "fluidgym_amd", "csrc", "Makefile")).read()
    assert all("fg_planespectra.hip" in line for line in mk.splitlines() if line.startswith(("SRCS =", "F64_SRCS =")))
    one = ctypes.c_void_p(64)          # never dereferenced: every call below fails its checks before anything touches the device
    ptrs = (ctypes.c_void_p * 5)(*([64] * 5))
    holes = (ctypes.c_void_p * 5)(64, 64, None, 64, 64)
    big = (ctypes.c_int64 * 5)(*([1 << 40] * 5))
    strides = (ctypes.c_int64 * 5)(*([4 * 4 * 8] * 5))
    short = (ctypes.c_int64 * 5)(128, 128, 127, 128, 128)
    rows = (ctypes.c_int32 * 33)(*([1, 3] + [0] * 31))
    high = (ctypes.c_int32 * 2)(1, 4)
    low = (ctypes.c_int32 * 2)(-1, 0)
    for lib, item in ((L.load(), 4), (L.load_f64(), 8)):
        f = lib.fg_plane_spectra
        invalid = [
            (None, strides, 4, 1, 4, 4, 8, rows, 2, one, one),         # null tables
            (ptrs, None, 4, 1, 4, 4, 8, rows, 2, one, one),
            (ptrs, strides, 4, 1, 4, 4, 8, None, 2, one, one),
            (holes, strides, 4, 1, 4, 4, 8, rows, 2, one, one),        # a null channel
            (ptrs, strides, 4, 1, 4, 4, 8, rows, 2, None, one),        # null accumulators
            (ptrs, strides, 4, 1, 4, 4, 8, rows, 2, one, None),
            (ptrs, strides, 0, 1, 4, 4, 8, rows, 2, one, one),         # K outside 1..5
            (ptrs, strides, 6, 1, 4, 4, 8, rows, 2, one, one),
            (ptrs, strides, 4, 1, 4, 4, 8, rows, 0, one, one),         # n_planes outside 1..32
            (ptrs, strides, 4, 1, 4, 4, 8, rows, 33, one, one),
            (ptrs, strides, 4, 1, 4, 4, 8, high, 2, one, one),         # a plane index outside [0, ny)
            (ptrs, strides, 4, 1, 4, 4, 8, low, 2, one, one),
            (ptrs, strides, 4, 0, 4, 4, 8, rows, 2, one, one),         # non-positive extents
            (ptrs, strides, 4, 1, 0, 4, 8, rows, 2, one, one),
            (ptrs, strides, 4, 1, 4, -4, 8, rows, 2, one, one),
            (ptrs, strides, 4, 1, 4, 4, 0, rows, 2, one, one),
            (ptrs, short, 4, 1, 4, 4, 8, rows, 2, one, one),           # a batch stride below nz * ny * nx
        ]
        for args in invalid:
            assert f(*args, None) == -1, args
            assert b"fg_plane_spectra" in lib.fg_last_error()
        unsupported = [((8, 24), b"nx must be a power of two"), ((8, 1024), b"nx must be a power of two"), ((8, 4), b"nx must be"),
                       ((2, 16), b"nz must be 1 or a power of two"), ((512, 16), b"nz must be"), ((256, 512), b"160 KB of LDS")]
        if item == 8:
            unsupported.append(((256, 128), b"160 KB of LDS"))             # fits as floats, not as doubles
        for (nz, nx), rule in unsupported:
            assert f(ptrs, big, 4, 1, nz, 4, nx, rows, 2, one, one, None) == L.FG_ERR_UNSUPPORTED, (nz, nx)
            assert rule in lib.fg_last_error(), lib.fg_last_error()
            with pytest.raises(ValueError):
                check_extents(nz, nx, item)
