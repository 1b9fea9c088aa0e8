"""``fg_obs_noise_add`` alone on the GPU, held bit for bit to the NumPy checker (``tests/obs_noise_ref.py``): both
dtypes, both load forms, tails, strides with guard values, in-place, eight segments, non-finite inputs, counters and row ids."""
import ctypes

import numpy as np
import pytest
import torch

from fluidgym_amd import _lib as L
from tests import obs_noise_ref as R

pytestmark = pytest.mark.gpu

GUARD = 12345.0
# a lone tail lane, a tail of three, one quad, quad plus tail, one workgroup of 256 quads, the first lane and a tail of a second one
SIZES = (1, 3, 4, 5, 1024, 1025, 1031)
DTYPES = {0: (torch.float32, np.float32, np.uint32), 1: (torch.float64, np.float64, np.uint64)}


def _launch(dtype, rows, segs, counters, row_ids=None, seed=0x0123456789ABCDEF):
    """``segs``: dicts with ``src`` (host ``[rows, n]``), ``tag``, ``sigma`` and optionally ``src_stride`` / ``dst_stride`` (elements),
    ``offset`` (elements both bases are moved off their aligned allocation) and ``inplace``.  Every buffer is filled with GUARD around the
    rows.  Returns per segment (dst buffer on the host, offset, dst stride, src buffer before, src buffer after)."""
    tdt, ndt, _ = DTYPES[dtype]
    dev = torch.device("cuda", 0)
    c_segs, keep = [], []
    for s in segs:
        src = np.asarray(s["src"], dtype=ndt).reshape(rows, -1)
        n = src.shape[1]
        ss, ds, off = s.get("src_stride", n), s.get("dst_stride", n), s.get("offset", 0)
        sbuf = np.full(off + rows * ss + 5, GUARD, dtype=ndt)
        for r in range(rows):
            sbuf[off + r * ss: off + r * ss + n] = src[r]
        st = torch.from_numpy(sbuf).to(dev)
        if s.get("inplace"):
            assert ds == ss
            dt = st
        else:
            dt = torch.full((off + rows * ds + 5,), GUARD, dtype=tdt, device=dev)
        assert st.data_ptr() % 16 == 0 and dt.data_ptr() % 16 == 0
        esz = st.element_size()
        c_segs.append(L.FgNoiseSegment(st.data_ptr() + off * esz, dt.data_ptr() + off * esz, ss, ds, n, s["tag"], s["sigma"]))
        keep.append((st, dt, off, ds, sbuf, n))
    ct = torch.from_numpy(np.asarray(counters, dtype=np.uint32).reshape(rows, 2).view(np.int32).copy()).to(dev)
    it = None if row_ids is None else torch.tensor(list(row_ids), dtype=torch.int32, device=dev)
    arr = (L.FgNoiseSegment * len(c_segs))(*c_segs)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    L.check(L.load().fg_obs_noise_add(arr, len(c_segs), rows, dtype, seed, ctypes.c_void_p(ct.data_ptr()),
                                      None if it is None else ctypes.c_void_p(it.data_ptr()), stream))
    torch.cuda.synchronize(dev)
    assert np.array_equal(ct.cpu().numpy().view(np.uint32), np.asarray(counters, dtype=np.uint32).reshape(rows, 2))     # read only
    return [(dt.cpu().numpy(), off, ds, sbuf, st.cpu().numpy(), n) for st, dt, off, ds, sbuf, n in keep]


def _check(dtype, rows, segs, counters, row_ids=None, seed=0x0123456789ABCDEF):
    """Launch, then: every row equals the checker bit for bit, every other element of the dst buffer is still GUARD, and a src buffer
    that is not also the dst is unchanged."""
    _, ndt, bits = DTYPES[dtype]
    got = _launch(dtype, rows, segs, counters, row_ids, seed)
    want = R.noise_add(segs, rows, counters, row_ids, seed, dtype)
    for s, (dbuf, off, ds, sbuf, sbuf_after, n), w in zip(segs, got, want):
        mask = np.ones(dbuf.shape, dtype=bool)
        for r in range(rows):
            lo = off + r * ds
            bad = np.nonzero(dbuf[lo: lo + n].view(bits) != w[r].view(bits))[0]
            assert bad.size == 0, (f"tag {s['tag']} n {n} row {r}: {bad.size} elements differ, first at {bad[0]}: "
                                   f"{dbuf[lo + bad[0]]!r} != {w[r][bad[0]]!r}")
            mask[lo: lo + n] = False
        assert np.all(dbuf[mask] == GUARD), f"tag {s['tag']} n {n}: a guard value between or after the rows was written"
        if not s.get("inplace"):
            assert np.array_equal(sbuf_after.view(bits), sbuf.view(bits)), "the source was written"
    return got


def _rows(rng, rows, n):
    return rng.standard_normal((rows, n))


def _counters(rows):
    return np.array([[3 + r, 7 * r + 1] for r in range(rows)], dtype=np.uint32)


@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("dtype", [0, 1])
def test_sizes_in_both_load_forms(dtype, rows):
    """Every size, (a) rows packed back to back on an aligned base -- the 16-byte form whenever the row pitch allows it, the scalar form
    otherwise and for the tail quad -- and (b) one element off 16-byte alignment, which forces the scalar form."""
    rng = np.random.default_rng(10 * dtype + rows)
    for n in SIZES:
        for offset in (0, 1):
            _check(dtype, rows, [dict(src=_rows(rng, rows, n), tag=1, sigma=0.25, offset=offset)], _counters(rows))


@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("dtype", [0, 1])
def test_strides_larger_than_n_leave_the_gaps_alone(dtype, rows):
    """src and dst pitches larger than n and different from each other: multiples of four elements (16-byte form) and odd ones (scalar
    form); the guard values between and after the rows stay."""
    rng = np.random.default_rng(20 * dtype + rows)
    for n in SIZES:
        up = (n + 3) // 4 * 4
        for ss, ds in ((up + 4, up + 8), (n + 3, n + 1)):
            _check(dtype, rows, [dict(src=_rows(rng, rows, n), tag=2, sigma=1.5, src_stride=ss, dst_stride=ds)], _counters(rows))


@pytest.mark.parametrize("dtype", [0, 1])
def test_in_place(dtype):
    rng = np.random.default_rng(3)
    for n, stride, offset in ((1031, 1032, 0), (1031, 1031, 0), (5, 8, 1), (1024, 1024, 0)):
        _check(dtype, 3, [dict(src=_rows(rng, 3, n), tag=9, sigma=0.5, src_stride=stride, dst_stride=stride, offset=offset, inplace=True)],
               _counters(3))


@pytest.mark.parametrize("dtype", [0, 1])
def test_eight_segments_in_one_launch(dtype):
    """Different n (so most chunks of the grid belong to the longest segment only), tags and sigmas, one sigma = 0 (which still runs the
    arithmetic: the result is src + 0 z), one in place, one off alignment."""
    rng = np.random.default_rng(4)
    ns = (1, 1031, 4, 2050, 5, 1024, 3, 260)
    segs = [dict(src=_rows(rng, 3, n), tag=t, sigma=s) for n, t, s in zip(ns, (0, 1, 2, 3, 127, 128, 200, 255),
                                                                           (0.1, 1.0, 0.0, 2.5, 1e-3, 0.3, 7.0, 1e3))]
    segs[3].update(src_stride=2052, dst_stride=2052, inplace=True)
    segs[7].update(offset=1)
    got = _check(dtype, 3, segs, _counters(3))
    dbuf, off, ds, sbuf, _, n = got[2]
    assert np.array_equal(dbuf[:3 * 4], sbuf[:3 * 4])        # sigma = 0: the source's bits (no -0.0 or NaN among them)


@pytest.mark.parametrize("dtype", [0, 1])
def test_non_finite_sources(dtype):
    rng = np.random.default_rng(5)
    src = _rows(rng, 2, 13)
    src[0, [0, 5, 12]] = [np.nan, np.inf, -np.inf]
    src[1, [3, 4, 8]] = [-np.inf, np.nan, np.inf]
    got = _check(dtype, 2, [dict(src=src, tag=0, sigma=1.0)], _counters(2))
    out = got[0][0][:26].reshape(2, 13)
    assert np.isnan(out[0, 0]) and out[0, 5] == np.inf and out[0, 12] == -np.inf and np.isnan(out[1, 4])
    assert np.isfinite(out[0, 1:5]).all()


@pytest.mark.parametrize("dtype", [0, 1])
def test_counters_seed_and_row_ids(dtype):
    """Each of seed, episode word, step word, tag and row id changes the numbers; rows [5, 2] with their counters are rows 5 and 2 of a
    six-row launch; the full range of the words is taken as unsigned."""
    rng = np.random.default_rng(6)
    n = 37
    src6 = _rows(rng, 6, n)
    c6 = np.array([[1, 0], [1, 1], [0xFFFFFFFF, 0x80000000], [2, 5], [7, 7], [123456789, 4000000000]], dtype=np.uint64).astype(np.uint32)
    full = _check(dtype, 6, [dict(src=src6, tag=4, sigma=1.0)], c6)[0][0][: 6 * n].reshape(6, n)
    part = _check(dtype, 2, [dict(src=src6[[5, 2]], tag=4, sigma=1.0)], c6[[5, 2]], row_ids=[5, 2])[0][0][: 2 * n].reshape(2, n)
    assert np.array_equal(part.view(DTYPES[dtype][2]), full[[5, 2]].view(DTYPES[dtype][2]))
    base = dict(src=src6[:1], tag=4, sigma=1.0)
    ref = _check(dtype, 1, [base], [[1, 0]])[0][0][:n]
    assert np.array_equal(ref, full[0])
    for kw in (dict(seed=0x0123456789ABCDEE), dict(seed=0x0023456789ABCDEF), dict(counters=[[2, 0]]), dict(counters=[[1, 1]]),
               dict(row_ids=[1]), dict(segs=[dict(base, tag=5)])):
        args = dict(segs=[base], counters=[[1, 0]])
        args.update(kw)
        other = _check(dtype, 1, **args)[0][0][:n]
        assert not np.array_equal(other, ref), kw
