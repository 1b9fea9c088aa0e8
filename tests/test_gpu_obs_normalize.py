"""``fg_obs_normalize`` and ``fg_obs_return_normalize`` alone on the GPU against the NumPy checker (``tests/obs_normalize_ref.py``;
DESIGN.md section 6o).  The checker sums in NumPy's order, so records and outputs are held to the bounds derived in its docstring
(``R.C = 8``); what the kernels promise bit for bit -- the same sequence twice, aligned and misaligned bases, 16-byte and single-element
loads, an explicit full row list and NULL, rows that are not listed -- is compared with ``torch.equal``.

Test data: |x| <= 8, every slot's standard deviation at least 0.25 (rows 0 and 1 of a column lie 2 apart, the rest is uniform over a
width of 8), plus one column that is constant over all rows."""
import ctypes

import numpy as np
import pytest
import torch

from fluidgym_amd import _lib as L
from fluidgym_amd.wrappers.normalize import normalize_tensors
from tests import obs_normalize_ref as R

pytestmark = pytest.mark.gpu

GUARD = 12345.0
EPS = 1e-8
DTYPES = {0: (torch.float32, np.float32), 1: (torch.float64, np.float64)}
# a lone tail lane, a tail of three, one quad, quad plus tail, below / at / above a 64-quad tile, several tiles and a tail of three
SIZES = (1, 3, 4, 5, 255, 256, 257, 1027)


def _dev():
    return torch.device("cuda", 0)


def _data(rng, rows, n, ndt, const_col=True):
    x = rng.uniform(-4.0, 4.0, (rows, n)) + rng.uniform(-3.0, 3.0, (1, n))
    if rows > 1:
        x[1] = x[0] + np.where(x[0] > 0, -2.0, 2.0)
    if const_col and n > 1:
        x[:, n // 2] = 1.5
    return x.astype(ndt)


def _records(ns, pooled=False):
    return [(torch.zeros(1 if pooled else n, dtype=torch.float64, device=_dev()), torch.zeros(1 if pooled else n, dtype=torch.float64,
                                                                                           device=_dev())) for n in ns]


def _launch(dtype, xs, recs, n_before, *, update=True, row_list=None, offset=0, pad=0, pooled=False, clip=0.0, inplace=False, eps=EPS):
    """One ``fg_obs_normalize`` call on the host arrays ``xs`` (``[rows, n]`` each, one segment each) with the device records ``recs``.
    ``offset``: elements both bases are moved off their 16-byte-aligned allocation; ``pad``: elements added to both row strides.  Checks
    that nothing outside the rows of a dst buffer was written and that a src that is not the dst is unchanged; returns the outputs."""
    ndt = DTYPES[dtype][1]
    rows = xs[0].shape[0]
    c_segs, keep = [], []
    for x, (mean, m2) in zip(xs, recs):
        n = x.shape[1]
        stride = n + pad
        sbuf = np.full(offset + rows * stride + 5, GUARD, dtype=ndt)
        for r in range(rows):
            sbuf[offset + r * stride: offset + r * stride + n] = x[r]
        st = torch.from_numpy(sbuf).to(_dev())
        dt = st if inplace else torch.full_like(st, GUARD)
        assert st.data_ptr() % 16 == 0 and dt.data_ptr() % 16 == 0
        esz = st.element_size()
        c_segs.append(L.FgNormSegment(st.data_ptr() + offset * esz, dt.data_ptr() + offset * esz, stride, stride, n, 1 if pooled else 0,
                                      mean.data_ptr(), m2.data_ptr()))
        keep.append((st, dt, sbuf, n, stride))
    rl = None if row_list is None else torch.tensor(list(row_list), dtype=torch.int32, device=_dev())
    m = rows if rl is None else int(rl.numel())
    arr = (L.FgNormSegment * len(c_segs))(*c_segs)
    stream = ctypes.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream)
    L.check(L.load().fg_obs_normalize(arr, len(c_segs), rows, dtype, n_before, m if update else 0,
                                      None if rl is None else ctypes.c_void_p(rl.data_ptr()), 0 if rl is None else m, 1 if update else 0,
                                      eps, clip, stream))
    torch.cuda.synchronize(_dev())
    outs = []
    for st, dt, sbuf, n, stride in keep:
        dbuf = dt.cpu().numpy()
        mask = np.ones(dbuf.shape, dtype=bool)
        out = np.empty((rows, n), ndt)
        for r in range(rows):
            lo = offset + r * stride
            out[r] = dbuf[lo: lo + n]
            mask[lo: lo + n] = False
        assert np.all(dbuf[mask] == GUARD), f"n {n}: a value between or after the rows was written"
        if not inplace:
            assert np.array_equal(st.cpu().numpy(), sbuf), "the source was written"
        outs.append(out)
    return outs


def _hold_record(rec, ref, what):
    """mean and M2 within C N 2^-52 of their natural scales 8 and 64 N, N the values merged (derivation: obs_normalize_ref)."""
    count = ref.n                      # the checker counts values: rows, or rows x n in a pooled slot
    t_mean, t_m2 = R.tolerances(count)
    d_mean = float(np.max(np.abs(rec[0].cpu().numpy() - ref.mean)))
    d_m2 = float(np.max(np.abs(rec[1].cpu().numpy() - ref.m2)))
    print(f"{what}: N {count}  |mean - ref| {d_mean:.3e} (bound {t_mean:.3e})  |M2 - ref| {d_m2:.3e} (bound {t_m2:.3e})")
    assert d_mean <= t_mean and d_m2 <= t_m2, what


def _hold_output(out, x, ref, ndt, what, clip=None):
    """fp32: 2^-23 max(1, |ref|), one rounding dominates; fp64: the propagated record error times rstd_max = 4 (obs_normalize_ref)."""
    want = ref.apply(x, EPS, clip)
    assert out.dtype == want.dtype == ndt
    tol = R.output_tolerance(want, ref.n, ndt)
    dev = np.abs(out.astype(np.float64) - want.astype(np.float64))
    print(f"{what}: worst |y - ref| / bound {float(np.max(dev / tol)):.3f}")
    assert np.all(dev <= tol), what


def _same(a, b):
    return all(torch.equal(torch.from_numpy(p), torch.from_numpy(q)) for p, q in zip(a, b))


def _same_records(a, b):
    return all(torch.equal(p[0], q[0]) and torch.equal(p[1], q[1]) for p, q in zip(a, b))


# ------------------------------------------------------------------------------------------------ element slots
@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("rows", [1, 3, 65, 257])
def test_element_shapes_alignment_and_strides(rows, dtype):
    """All eight sizes in one call of eight segments, at an aligned and at a misaligned base, with the row stride equal to n and larger:
    the 16-byte and the single-element load forms.  Every form within the bounds of the checker, and all four bit for bit the same."""
    ndt = DTYPES[dtype][1]
    rng = np.random.default_rng(100 * rows + dtype)
    xs = [_data(rng, rows, n, ndt) for n in SIZES]
    refs = [R.Record().update(x) for x in xs]
    first = None
    # 16-byte words where n, base and pitch allow; a misaligned base: single elements; pitches that make other sizes wide (with tails)
    for offset, pad in ((0, 0), (1, 0), (0, 4), (0, 3), (0, 1)):
        recs = _records(SIZES)
        outs = _launch(dtype, xs, recs, 0, offset=offset, pad=pad)
        for n, x, rec, ref, out in zip(SIZES, xs, recs, refs, outs):
            _hold_record(rec, ref, f"rows {rows} n {n} offset {offset} pad {pad}")
            _hold_output(out, x, ref, ndt, f"rows {rows} n {n} offset {offset} pad {pad}")
            if n > 1:
                assert np.all(out[:, n // 2] == 0.0), "a column constant over all rows must give exactly 0"
        if first is None:
            first = (outs, recs)
        else:
            assert _same(outs, first[0]) and _same_records(recs, first[1]), f"offset {offset} pad {pad} differs from the aligned form"


@pytest.mark.parametrize("dtype", [0, 1])
def test_many_rows_of_few_elements(dtype):
    """4 099 rows of 6 elements: 1024 row lanes per quad column, five rows in the longest lane."""
    ndt = DTYPES[dtype][1]
    x = _data(np.random.default_rng(7), 4099, 6, ndt)
    ref = R.Record().update(x)
    recs = _records([6])
    out = _launch(dtype, [x], recs, 0)[0]
    _hold_record(recs[0], ref, "rows 4099 n 6")
    _hold_output(out, x, ref, ndt, "rows 4099 n 6")
    recs2 = _records([6])
    out2 = _launch(dtype, [x], recs2, 0, offset=1)[0]
    assert _same([out], [out2]) and _same_records(recs, recs2)


def test_nine_tensors_through_the_python_helper_take_two_calls():
    rng = np.random.default_rng(8)
    ns = (2, 7, 16, 33, 64, 5, 100, 12, 9)
    xs = [_data(rng, 5, n, np.float32) for n in ns]
    recs = _records(ns)
    outs = normalize_tensors([torch.from_numpy(x).to(_dev()).reshape(5, 1, n) for x, n in zip(xs, ns)], [r[0] for r in recs],
                             [r[1] for r in recs], 5, 0, update=True, epsilon=EPS)
    torch.cuda.synchronize()
    assert len(outs) == 9
    for x, n, rec, out in zip(xs, ns, recs, outs):
        ref = R.Record().update(x)
        assert out.shape == (5, 1, n)
        _hold_record(rec, ref, f"helper n {n}")
        _hold_output(out.reshape(5, n).cpu().numpy(), x, ref, np.float32, f"helper n {n}")


@pytest.mark.parametrize("dtype", [0, 1])
def test_row_lists(dtype):
    """One row, a strict subset, all rows given explicitly (= NULL bit for bit); rows that are not listed do not influence the record."""
    ndt = DTYPES[dtype][1]
    rng = np.random.default_rng(21)
    ns = (5, 64)
    xs = [_data(rng, 6, n, ndt) for n in ns]
    base_refs = [R.Record().update(_data(rng, 4, n, ndt, const_col=False)) for n in ns]     # a record to merge into

    def start():
        recs = _records(ns)
        for (mean, m2), ref in zip(recs, base_refs):
            mean.copy_(torch.from_numpy(ref.mean)), m2.copy_(torch.from_numpy(ref.m2))
        return recs

    for rows_sel in ([3], [1, 4]):
        recs = start()
        outs = _launch(dtype, xs, recs, 4, row_list=rows_sel)
        spoiled = [x.copy() for x in xs]
        others = [r for r in range(6) if r not in rows_sel]
        for s in spoiled:
            s[others] = 1e30
        recs_spoiled = start()
        outs_spoiled = _launch(dtype, spoiled, recs_spoiled, 4, row_list=rows_sel)
        assert _same_records(recs, recs_spoiled), "a row that is not listed influenced the record"
        assert _same([o[rows_sel] for o in outs], [o[rows_sel] for o in outs_spoiled])
        for x, n, rec, base, out in zip(xs, ns, recs, base_refs, outs):
            ref = R.Record()
            ref.n, ref.mean, ref.m2 = base.n, base.mean.copy(), base.m2.copy()
            ref.update(x, rows=rows_sel)
            assert ref.n == 4 + len(rows_sel)
            _hold_record(rec, ref, f"rows {rows_sel} n {n}")
            _hold_output(out, x, ref, ndt, f"rows {rows_sel} n {n}")       # every row is normalised
    recs_null, recs_all = start(), start()
    outs_null = _launch(dtype, xs, recs_null, 4)
    outs_all = _launch(dtype, xs, recs_all, 4, row_list=range(6))
    assert _same(outs_null, outs_all) and _same_records(recs_null, recs_all)


# ------------------------------------------------------------------------------------------------ pooled slots
@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("rows, n", [(1, 1), (3, 85), (41, 25), (8, 625)])
def test_pooled_slots(rows, n, dtype):
    """rows x n = 1, 255, 1 025, 5 000 values in one scalar slot: two updates and a row list, both load forms bit for bit."""
    ndt = DTYPES[dtype][1]
    rng = np.random.default_rng(rows * n)
    x1, x2 = _data(rng, rows, n, ndt, const_col=False), _data(rng, rows, n, ndt, const_col=False)
    if rows * n == 1:
        x2 = np.where(x1 > 0, x1 - 2, x1 + 2).astype(ndt)         # two values in the slot: keep them 2 apart
    sel = list(range(0, rows, 2))
    forms = []
    for offset in (0, 1):
        recs = _records([n], pooled=True)
        ref = R.Record(pooled=True).update(x1)
        o1 = _launch(dtype, [x1], recs, 0, pooled=True, offset=offset)[0]
        _hold_record(recs[0], ref, f"pooled {rows} x {n} first")
        _hold_output(o1, x1, ref, ndt, f"pooled {rows} x {n} first")
        ref.update(x2, rows=sel)
        o2 = _launch(dtype, [x2], recs, rows, pooled=True, offset=offset, row_list=sel)[0]
        _hold_record(recs[0], ref, f"pooled {rows} x {n} second")
        _hold_output(o2, x2, ref, ndt, f"pooled {rows} x {n} second")
        kept = (recs[0][0].clone(), recs[0][1].clone())
        o3 = _launch(dtype, [x1], recs, rows + len(sel), pooled=True, offset=offset, update=False)[0]     # frozen: the record stays
        assert _same_records([kept], recs)
        _hold_output(o3, x1, ref, ndt, f"pooled {rows} x {n} frozen")
        forms.append((o1, o2, o3, recs))
    assert _same(forms[0][:3], forms[1][:3]) and _same_records(forms[0][3], forms[1][3])


def test_pooled_and_element_rows_count_consistently():
    """The kernel takes n in rows for both kinds of slot: a pooled record of n_before rows holds n_before x n values."""
    x = _data(np.random.default_rng(2), 4, 10, np.float32, const_col=False)
    recs = _records([10], pooled=True)
    _launch(0, [x], recs, 0, pooled=True)
    _launch(0, [x], recs, 4, pooled=True)
    ref = R.Record(pooled=True).update(x).update(x)
    assert ref.n == 80
    _hold_record(recs[0], ref, "pooled twice")


# ------------------------------------------------------------------------------------------------ sequences
def _sequence(dtype, inplace=False, clip=0.0, offset=0):
    """Three updates of 5, 2 and 9 rows with a frozen call in between: (outputs of the four calls, records, checker records)."""
    ndt = DTYPES[dtype][1]
    rng = np.random.default_rng(31)
    ns = (9, 130)
    recs = _records(ns)
    refs = [R.Record() for _ in ns]
    n_rows, outs_all, xs_all = 0, [], []
    for step, rows in enumerate((5, 2, None, 9)):
        if rows is None:                                           # frozen: normalise the first batch again, the record must not move
            kept = [(a.clone(), b.clone()) for a, b in recs]
            outs = _launch(dtype, xs_all[0], recs, n_rows, update=False, inplace=inplace, clip=clip, offset=offset)
            assert _same_records(kept, recs), "a frozen call moved the record"
            xs = xs_all[0]
        else:
            xs = [_data(rng, rows, n, ndt) for n in ns]
            for ref, x in zip(refs, xs):
                ref.update(x)
            outs = _launch(dtype, xs, recs, n_rows, inplace=inplace, clip=clip, offset=offset)
            n_rows += rows
        for n, x, rec, ref, out in zip(ns, xs, recs, refs, outs):
            _hold_record(rec, ref, f"step {step} n {n}")
            _hold_output(out, x, ref, ndt, f"step {step} n {n} clip {clip}", clip=clip or None)
            assert np.all(out[:, n // 2] == 0.0)
            if clip:
                assert np.max(np.abs(out)) <= clip
        outs_all.append(outs)
        xs_all.append(xs)
    return outs_all, recs


@pytest.mark.parametrize("dtype", [0, 1])
def test_sequences_repeat_and_do_not_depend_on_the_form(dtype):
    a_out, a_rec = _sequence(dtype)
    b_out, b_rec = _sequence(dtype)
    assert all(_same(p, q) for p, q in zip(a_out, b_out)) and _same_records(a_rec, b_rec), "the same sequence twice differs"
    c_out, c_rec = _sequence(dtype, offset=1)
    assert all(_same(p, q) for p, q in zip(a_out, c_out)) and _same_records(a_rec, c_rec), "the misaligned sequence differs"
    d_out, d_rec = _sequence(dtype, inplace=True)
    assert all(_same(p, q) for p, q in zip(a_out, d_out)) and _same_records(a_rec, d_rec), "dst == src differs"
    e_out, e_rec = _sequence(dtype, clip=1.0)
    assert _same_records(a_rec, e_rec), "the clip moved the record"
    assert any(np.max(np.abs(o)) > 1.0 for outs in a_out for o in outs)       # the clip had something to do


# ------------------------------------------------------------------------------------------------ the return record
def _return_step(dtype, reward, G, stats, n_before, gamma, update=True, clip=0.0):
    tdt, _ = DTYPES[dtype]
    r = torch.from_numpy(reward).to(_dev())
    out = torch.empty_like(r)
    p = ctypes.c_void_p
    stream = p(torch.cuda.current_stream(_dev()).cuda_stream)
    L.check(L.load().fg_obs_return_normalize(p(r.data_ptr()), p(out.data_ptr()), p(G.data_ptr()), p(stats.data_ptr()), reward.shape[0],
                                             dtype, gamma, n_before, EPS, clip, 1 if update else 0, stream))
    torch.cuda.synchronize(_dev())
    assert out.dtype == tdt and torch.equal(r.cpu(), torch.from_numpy(reward))
    return out.cpu().numpy()


def _hold_return(out, want, G, stats, ref, ndt, what):
    """|reward| <= 8 and three steps at gamma <= 1 keep |G| <= 24: the record's bounds at that scale; G itself is two roundings."""
    count = ref.rec.n
    t_mean, t_m2 = R.tolerances(count, x_max=24.0)
    g = G.cpu().numpy()
    assert np.all(np.abs(g - ref.G) <= 4 * 2.0 ** -52 * 24.0), what
    s = stats.cpu().numpy()
    print(f"{what}: N {count} |mean - ref| {abs(s[0] - ref.rec.mean):.3e} ({t_mean:.3e}) |M2 - ref| {abs(s[1] - ref.rec.m2):.3e} ({t_m2:.3e})")
    assert abs(s[0] - ref.rec.mean) <= t_mean and abs(s[1] - ref.rec.m2) <= t_m2, what
    assert np.all(np.abs(out.astype(np.float64) - want.astype(np.float64)) <= _return_tolerance(want, count, ndt)), what


def _return_tolerance(want, count, ndt):
    """fp32: one rounding; fp64: y = reward rstd moves by |y| rstd^2 dvar / 2 with rstd <= 4, dvar = dM2 / N, plus four roundings."""
    want = np.abs(want.astype(np.float64))
    if ndt == np.float32:
        return 2.0 ** -23 * np.maximum(1.0, want)
    return want * (R.RSTD_MAX ** 2 / 2.0) * (R.tolerances(count, x_max=24.0)[1] / count) + 4.0 * 2.0 ** -52 * want


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("gamma", [0.0, 0.99, 1.0])
@pytest.mark.parametrize("rows", [1, 5, 256, 4099])
def test_return_normalize(rows, gamma, dtype):
    ndt = DTYPES[dtype][1]
    rng = np.random.default_rng(rows + int(100 * gamma))
    G = torch.zeros(rows, dtype=torch.float64, device=_dev())
    stats = torch.zeros(2, dtype=torch.float64, device=_dev())
    ref = R.ReturnRecord(rows, gamma)
    n = 0
    for step in range(3):
        reward = (rng.uniform(1.0, 8.0, rows) * rng.choice([-1.0, 1.0], rows)).astype(ndt)
        want = ref.step(reward, EPS)
        out = _return_step(dtype, reward, G, stats, n, gamma)
        n += rows
        if ref.rec.m2 > 0:
            assert ref.rec.m2 / ref.rec.n >= 0.0625      # the bound's premise: a standard deviation of at least 0.25
        _hold_return(out, want, G, stats, ref, ndt, f"rows {rows} gamma {gamma} step {step}")
    # update = 0: G advances, the record's bits stay
    kept = stats.clone()
    reward = rng.uniform(-8.0, 8.0, rows).astype(ndt)
    want = ref.step(reward, EPS, update=False, clip=0.5)
    out = _return_step(dtype, reward, G, stats, n, gamma, update=False, clip=0.5)
    assert torch.equal(stats, kept)
    assert np.all(np.abs(G.cpu().numpy() - ref.G) <= 4 * 2.0 ** -52 * 32.0) and np.max(np.abs(out)) <= 0.5
    assert np.all(np.abs(out.astype(np.float64) - want.astype(np.float64)) <= _return_tolerance(want, ref.rec.n, ndt))


def test_return_zeroing_rows_changes_exactly_their_contributions():
    rows, gamma = 5, 0.9
    rng = np.random.default_rng(4)
    r1, r2 = (rng.uniform(1.0, 8.0, rows).astype(np.float32) for _ in range(2))
    runs = []
    for zero in (None, [1, 3]):
        G = torch.zeros(rows, dtype=torch.float64, device=_dev())
        stats = torch.zeros(2, dtype=torch.float64, device=_dev())
        ref = R.ReturnRecord(rows, gamma)
        ref.step(r1, EPS)
        _return_step(0, r1, G, stats, 0, gamma)
        if zero:
            G[torch.tensor(zero, device=_dev())] = 0.0
            ref.G[zero] = 0.0
        want = ref.step(r2, EPS)
        out = _return_step(0, r2, G, stats, rows, gamma)
        _hold_return(out, want, G, stats, ref, np.float32, f"zeroed {zero}")
        runs.append(G.cpu().numpy())
    assert np.array_equal(runs[1][[1, 3]], r2[[1, 3]].astype(np.float64))        # a fresh return: gamma * 0 + reward
    assert np.array_equal(runs[0][[0, 2, 4]], runs[1][[0, 2, 4]]) and not np.any(runs[0][[1, 3]] == runs[1][[1, 3]])
