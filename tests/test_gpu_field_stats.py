"""``fg_field_summary`` (csrc/fg_fieldstats.hip) and ``FieldSummary`` on the GPU against NumPy in fp64: exact min / max / counts, the
sum bit-equal to the host evaluation of the exact accumulator, histograms integer-equal to the NumPy bin expression, every env
independent of its batch, non-finite cells counted and kept out, and the growing range of ``FieldSummary`` against one
``np.histogram`` of everything it saw."""
import ctypes
import math

import numpy as np
import pytest
import torch

from fluidgym_amd import _lib as L
from fluidgym_amd.simulation.field_stats import FieldSummary, HostFieldSummary, bin_index

pytestmark = pytest.mark.gpu
D = ctypes.POINTER(ctypes.c_double)
# (library, (B, C, n)): one cell; odd n with an unaligned second channel; several workgroups per env plus a tail; the fp64 library
CASES = [("f32", (1, 1, 1)), ("f32", (3, 2, 1031)), ("f32", (2, 3, 70001)), ("f64", (2, 2, 1031))]
IDS = [f"{k}-{'x'.join(map(str, s))}" for k, s in CASES]


def _lib(kind):
    return L.load_f64() if kind == "f64" else L.load()


def _data(kind, shape, seed=0):
    """Seeded normal data with negative values, in the library's element type."""
    x = 3.0 * np.random.default_rng(seed).standard_normal(shape)
    return x.astype(np.float64 if kind == "f64" else np.float32)


def _host_sum(kind, values):
    v = np.ascontiguousarray(values, np.float64)
    out = ctypes.c_double()
    L.check(_lib(kind).fg_dacc_host_sum(v.ctypes.data_as(D), v.size, 0.0, ctypes.byref(out)))
    return out.value


def _summary(kind, x, channel, lo=0.0, width=1.0, nbins=0, hist=None, moments=True):
    """One call: returns (moments [B,3] f64, counts [B,2] i64, hist [B,nbins] i64) as device tensors."""
    t = torch.as_tensor(x).cuda().contiguous() if not isinstance(x, torch.Tensor) else x
    B, C, n = t.shape
    p = lambda a: ctypes.c_void_p(a.data_ptr()) if a is not None else ctypes.c_void_p(None)
    work = torch.empty(B * L.FG_FIELD_SUMMARY_WORK_BYTES, dtype=torch.uint8, device="cuda") if moments else None
    mom = torch.full((B, 3), -7.0, dtype=torch.float64, device="cuda") if moments else None
    cnt = torch.full((B, 2), -7, dtype=torch.int64, device="cuda") if moments else None
    if nbins and hist is None:
        hist = torch.zeros(B, nbins, dtype=torch.int64, device="cuda")
    lib = _lib(kind)
    L.check(lib.fg_field_summary(p(t), B, C, n, -1 if channel is None else channel, p(work), p(mom), p(cnt), lo, width,
                                 nbins if nbins else 1, p(hist if nbins else None),
                                 ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), lib=lib)
    torch.cuda.synchronize()
    return mom, cnt, hist


def _magnitude(x):
    acc = np.zeros((x.shape[0], x.shape[2]))
    for c in range(x.shape[1]):                      # ascending channel order, fp64
        v = x[:, c].astype(np.float64)
        acc = acc + v * v
    return np.sqrt(acc)


def _off_the_edges(x, lo, width):
    """Move every cell whose fp64 magnitude lies within 1e-12 (relative) of a bin edge: a fused multiply-add in the kernel may
    round the sum of squares one ulp away from NumPy's, which must not decide a bin."""
    for _ in range(8):
        mag = _magnitude(x)
        q = (mag - lo) / width
        near = np.abs(q - np.rint(q)) * width <= 1e-12 * np.maximum(mag, abs(lo) + np.abs(np.rint(q)) * width)
        if not near.any():
            return x
        x[:, 0][near] = x[:, 0][near] * x.dtype.type(1.01) + x.dtype.type(1e-3)
    raise AssertionError("could not move the cells off the bin edges")


@pytest.mark.parametrize("kind,shape", CASES, ids=IDS)
def test_component_mode_is_exact(kind, shape):
    x = _data(kind, shape)
    B, C, n = shape
    ch = C - 1
    v = x[:, ch].astype(np.float64)
    lo, width, nbins = -4.0, 8.0 / 4096, 4096              # +-4 of a 3-sigma normal: both end bins collect clamped cells
    mom, cnt, hist = _summary(kind, x, ch, lo, width, nbins)
    mom, cnt, hist = mom.cpu().numpy(), cnt.cpu().numpy(), hist.cpu().numpy()
    for b in range(B):
        print(kind, shape, b, mom[b], cnt[b], v[b].min(), v[b].max(), math.fsum(v[b]))
        assert mom[b, 0] == v[b].min() and mom[b, 1] == v[b].max()
        assert cnt[b].tolist() == [n, 0]
        assert mom[b, 2] == _host_sum(kind, v[b])                                 # bit-equal to the host evaluation
        assert abs(mom[b, 2] - math.fsum(v[b])) <= 1e-12 * abs(math.fsum(v[b]))
        assert np.array_equal(hist[b], np.bincount(bin_index(v[b], lo, width, nbins), minlength=nbins))
    assert hist.sum() == B * n


@pytest.mark.parametrize("kind,shape", CASES, ids=IDS)
def test_magnitude_mode(kind, shape):
    B, C, n = shape
    lo, width, nbins = 0.0, 12.0 / 1000, 1000
    x = _off_the_edges(_data(kind, shape, seed=1), lo, width)
    mag = _magnitude(x)
    mom, cnt, hist = _summary(kind, x, None, lo, width, nbins)
    mom, cnt, hist = mom.cpu().numpy(), cnt.cpu().numpy(), hist.cpu().numpy()
    for b in range(B):
        print(kind, shape, b, mom[b], mag[b].min(), mag[b].max())
        assert abs(mom[b, 0] - mag[b].min()) <= 1e-15 * mag[b].min() and abs(mom[b, 1] - mag[b].max()) <= 1e-15 * mag[b].max()
        assert cnt[b].tolist() == [n, 0]
        assert abs(mom[b, 2] - math.fsum(mag[b])) <= 1e-12 * math.fsum(mag[b])
        assert np.array_equal(hist[b], np.bincount(bin_index(mag[b], lo, width, nbins), minlength=nbins))


@pytest.mark.parametrize("kind,shape", CASES[1:], ids=IDS[1:])
def test_an_env_does_not_depend_on_its_batch_and_launches_add(kind, shape):
    x = torch.as_tensor(_data(kind, shape, seed=2)).cuda()
    for ch in (None, 0, shape[1] - 1):
        mom, cnt, hist = _summary(kind, x, ch, -5.0, 0.01, 1024)
        for b in range(shape[0]):
            m1, c1, h1 = _summary(kind, x[b:b + 1].contiguous(), ch, -5.0, 0.01, 1024)
            assert torch.equal(m1[0], mom[b]) and torch.equal(c1[0], cnt[b]) and torch.equal(h1[0], hist[b])
        again = _summary(kind, x, ch, -5.0, 0.01, 1024, hist=hist.clone(), moments=False)[2]      # histogram job alone, adding
        assert torch.equal(again, 2 * hist)


@pytest.mark.parametrize("kind,shape", CASES[1:], ids=IDS[1:])
def test_non_finite_cells_are_counted_and_kept_out(kind, shape):
    clean = _data(kind, shape, seed=3)
    x = clean.copy()
    x[1, 0, 3], x[1, shape[1] - 1, 5], x[1, 0, 7] = np.nan, np.inf, -np.inf          # env 1 only
    for ch, bad_cells in ((0, [3, 7]), (None, [3, 5, 7])):
        ref = _summary(kind, clean, ch, -5.0, 0.01, 1024)
        got = _summary(kind, x, ch, -5.0, 0.01, 1024)
        for b in range(shape[0]):
            if b != 1:
                assert all(torch.equal(g[b], r[b]) for g, r in zip(got, ref))          # the other envs are unaffected
        keep = np.setdiff1d(np.arange(shape[2]), bad_cells)
        v = (_magnitude(x)[1] if ch is None else x[1, ch].astype(np.float64))[keep]
        mom, cnt, hist = (t.cpu().numpy() for t in got)
        assert cnt[1].tolist() == [keep.size, len(bad_cells)]
        if ch is None:
            assert mom[1, 0] == pytest.approx(v.min(), rel=1e-15) and mom[1, 1] == pytest.approx(v.max(), rel=1e-15)
        else:
            assert mom[1, 0] == v.min() and mom[1, 1] == v.max()
        assert abs(mom[1, 2] - math.fsum(v)) <= 1e-12 * abs(math.fsum(v)) and hist[1].sum() == keep.size
    # an env without a finite cell
    x[1] = np.nan
    mom, cnt, hist = (t.cpu().numpy() for t in _summary(kind, x, 0, -5.0, 0.01, 1024))
    assert np.isnan(mom[1, 0]) and np.isnan(mom[1, 1]) and mom[1, 2] == 0.0 and cnt[1].tolist() == [0, shape[2]] and hist[1].sum() == 0


def test_constant_field():
    x = np.full((2, 2, 5000), 2.5, np.float32)
    mom, cnt, hist = (t.cpu().numpy() for t in _summary("f32", x, 1, 0.0, 1.0, 8))
    assert mom.tolist() == [[2.5, 2.5, 12500.0]] * 2 and cnt.tolist() == [[5000, 0]] * 2
    assert hist.tolist() == [[0, 0, 5000, 0, 0, 0, 0, 0]] * 2
    fs = FieldSummary(nbins=64)
    fs.update(torch.as_tensor(x).cuda(), channel=1)
    assert np.count_nonzero(fs.histogram()) == 1 and fs.stats() == (2.5,) * 8


@pytest.mark.parametrize("dtype,channel,fused", [(torch.float32, 1, False), (torch.float32, 1, True), (torch.float64, None, False)],
                         ids=["f32-component", "f32-component-fused", "f64-magnitude"])
def test_field_summary_grows_its_range_both_ways(dtype, channel, fused):
    rng = np.random.default_rng(5)
    # (unequal sample sizes: no percentile of Stats falls into the empty gap between two clusters, where any value is "the" quantile)
    base = [rng.standard_normal((2, 2, n)) for n in (3001, 2003, 1009, 2501)]
    chunks = [base[0], 5.0 * base[1], 20.0 + base[2], base[3] - 50.0]                # the range grows up, then down
    chunks = [c.astype(np.float32 if dtype == torch.float32 else np.float64) for c in chunks]
    if channel is None:
        # every edge of every range the summary passes through lies on the lattice of the first one: keep the magnitudes off it
        first = HostFieldSummary(nbins=512)
        first.update(chunks[0])
        lattice = (first.range.lo, first.range.width)
        chunks = [_off_the_edges(c, *lattice) for c in chunks]
        again = HostFieldSummary(nbins=512)
        again.update(chunks[0])
        assert (again.range.lo, again.range.width) == lattice
    fs, twin = FieldSummary(nbins=512, per_env=True, fused=fused), HostFieldSummary(nbins=512, per_env=True)
    widths = []
    for c in chunks:
        fs.update(torch.as_tensor(c).cuda(), channel=channel)
        twin.update(c, channel=channel)
        widths.append((fs.range.lo, fs.range.width))
    assert len(set(widths)) >= 3 and widths[-1][1] > widths[0][1] and (channel is None or widths[-1][0] < widths[0][0])
    pooled = np.concatenate([(_magnitude(c) if channel is None else c[:, channel].astype(np.float64)) for c in chunks], axis=1)
    r = fs.range
    assert (r.lo, r.width) == (twin.range.lo, twin.range.width)
    h = fs.histogram()
    for b in range(2):
        assert np.array_equal(h[b], np.histogram(pooled[b], bins=r.nbins, range=(r.lo, r.hi))[0])
    assert np.array_equal(h, twin.histogram())
    for b, st in enumerate(fs.stats()):
        q = np.quantile(pooled[b], [0.05, 0.25, 0.5, 0.75, 0.95])
        print(dtype, channel, b, st, q, r.width)
        assert np.abs(np.array(st[3:]) - q).max() <= r.width
        assert st.min == pytest.approx(pooled[b].min(), rel=1e-15) and st.max == pytest.approx(pooled[b].max(), rel=1e-15)
        assert st.mean == pytest.approx(pooled[b].mean(), rel=1e-12)
    # pooled over the envs, merged from two halves
    a, b2 = FieldSummary(nbins=512), FieldSummary(nbins=512)
    for c in chunks[:2]:
        a.update(torch.as_tensor(c).cuda(), channel=channel)
    for c in chunks[2:]:
        b2.update(torch.as_tensor(c).cuda(), channel=channel)
    a.merge(b2)
    assert a.count == pooled.size and a.stats().max == pytest.approx(pooled.max(), rel=1e-15)
    assert abs(a.stats().p50 - np.quantile(pooled, 0.5)) <= 2 * a.range.width
