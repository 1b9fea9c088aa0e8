"""Plane histograms without a GPU: the checker (``tests/plane_hist_ref.py``) against ``np.histogram`` / ``np.histogram2d`` where
both rules agree exactly, the slot rules at the edges, the joint identities, ``HostPlaneHistograms`` against the checker, the
accessors on hand-made tables, every refusal of the Python layer and of ``fg_plane_histogram`` (no launch), and the env guard."""
import ctypes
import os
import re

import numpy as np
import pytest

import fluidgym_amd
from fluidgym_amd import _lib as L
from fluidgym_amd.simulation.plane_hist import HostPlaneHistograms, PlaneHistograms, bin_slots
from tests import plane_hist_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = (np.float32, np.float64)


def _centre_values(rng, bins, shape, dtype):
    """Values exactly at the centres of ``bins`` bins of [-1, 1] (``bins`` a power of two: centres, edges and scale are exact)."""
    return (-1.0 + (2.0 * rng.integers(0, bins, shape) + 1.0) / bins).astype(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bins", (2, 8, 64))
def test_checker_agrees_with_numpy_where_both_rules_are_exact(dtype, bins):
    rng = np.random.default_rng(bins)
    u, v = _centre_values(rng, bins, (2, 3, 4, 10), dtype), _centre_values(rng, bins, (2, 3, 4, 10), dtype)
    rows = [0, 2, 3]
    lo, scale = ref.tables(np.full((3, 2), -1.0), np.full((3, 2), 1.0), bins, dtype)
    assert scale[0, 0] == bins / 2
    jb = max(bins // 2, 2)
    counts, joint = ref.histogram([u, v], rows, lo, scale, bins, [(0, 1)], jb)
    for b in range(2):
        for r, y in enumerate(rows):
            for k, f in enumerate((u, v)):
                h, _ = np.histogram(f[b, :, y, :], bins=bins, range=(-1.0, 1.0))
                assert np.array_equal(counts[b, r, k, 1:bins + 1], h.astype(np.uint64))
                assert not counts[b, r, k, [0, bins + 1, bins + 2]].any()
            h2, _, _ = np.histogram2d(u[b, :, y, :].ravel(), v[b, :, y, :].ravel(), bins=jb, range=((-1.0, 1.0), (-1.0, 1.0)))
            assert np.array_equal(joint[b, r, 0, :-1].reshape(jb, jb), h2.astype(np.uint64)) and joint[b, r, 0, -1] == 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_slot_rules_at_the_edges(dtype):
    bins = 8
    up, down = lambda x: np.nextafter(dtype(x), dtype(np.inf)), lambda x: np.nextafter(dtype(x), dtype(-np.inf))
    # lo = 0: v - lo and the product with scale = 8 are exact, so the slots are those of the real numbers
    lo, hi = dtype(0.0), dtype(1.0)
    lo_r, scale = ref.tables(lo, hi, bins, dtype)
    v = np.array([lo, down(lo), up(lo), hi, down(hi), up(hi), np.inf, -np.inf, np.nan, 0.5, down(0.5), 1e30, -1e30], dtype)
    want = [1, 0, 1, bins + 1, bins, bins + 1, bins + 1, 0, bins + 2, 5, 4, bins + 1, 0]
    assert ref.slots(v, lo_r, scale, bins).tolist() == want
    assert bin_slots(v, lo_r, scale, bins).tolist() == want
    # lo = -1: the difference is rounded first.  One ulp below hi = 1 gives 2 - ulp / 2, a tie that rounds to even, 2: the value
    # counts as above; the largest negative number gives 1 - tiny = 1 and sits in the bin of 0.  That is the rule, not an accident.
    lo, hi = dtype(-1.0), dtype(1.0)
    lo_r, scale = ref.tables(lo, hi, bins, dtype)
    v = np.array([lo, down(lo), up(lo), hi, down(hi), up(hi), np.inf, -np.inf, np.nan, 0.0, down(0.0), 1e30, -1e30], dtype)
    want = [1, 0, 1, bins + 1, bins + 1, bins + 1, bins + 1, 0, bins + 2, 5, 5, bins + 1, 0]
    assert ref.slots(v, lo_r, scale, bins).tolist() == want
    assert bin_slots(v, lo_r, scale, bins).tolist() == want
    big = np.array([np.finfo(dtype).max, -np.finfo(dtype).max], dtype)                     # t overflows to +-inf: compared as a real
    assert ref.slots(big, lo_r, scale, bins).tolist() == [bins + 1, 0] == bin_slots(big, lo_r, scale, bins).tolist()


def _spread(rng, shape, dtype, nan_at=None):
    f = (rng.standard_normal(shape) * 1.5).astype(dtype)
    if nan_at is not None:
        f[nan_at] = np.nan
    return f


@pytest.mark.parametrize("dtype", DTYPES)
def test_joint_marginals_are_the_coarsened_counts(dtype):
    rng = np.random.default_rng(5)
    shape = (2, 3, 4, 33)
    f = [_spread(rng, shape, dtype, (0, 1, 2, 3)), _spread(rng, shape, dtype), _spread(rng, shape, dtype, (1, 0, 0, 0))]
    f[1][0, 0, 1, :3] = (np.inf, -np.inf, 7.0)
    bins, jb, rows, pairs = 12, 4, [0, 1, 2, 3], [(0, 1), (2, 2), (1, 2)]
    lo, scale = ref.tables(np.full((4, 3), -2.0), np.full((4, 3), 2.5), bins, dtype)
    counts, joint = ref.histogram(f, rows, lo, scale, bins, pairs, jb)
    cells = shape[1] * shape[3]
    assert (counts.sum(axis=-1) == cells).all() and (joint.sum(axis=-1) == cells).all()
    assert counts[0, 2, 0, bins + 2] == 1 and counts[1, 0, 2, bins + 2] == 1 and counts[..., bins + 2].sum() == 2
    assert ref.slots(f[1][0, 0, 1, :3], lo[1, 1], scale[1, 1], bins).tolist() == [bins + 1, 0, bins + 1]
    for b in range(2):
        for r in range(4):
            s = [ref.slots(np.ascontiguousarray(f[k][b, :, r, :]), lo[r, k], scale[r, k], bins).ravel() for k in range(3)]
            for p, (ia, ib) in enumerate(pairs):
                both = (s[ia] >= 1) & (s[ia] <= bins) & (s[ib] >= 1) & (s[ib] <= bins)
                t = joint[b, r, p, :-1].reshape(jb, jb)
                assert np.array_equal(t.sum(axis=1), np.bincount((s[ia][both] - 1) // 3, minlength=jb).astype(np.uint64))
                assert np.array_equal(t.sum(axis=0), np.bincount((s[ib][both] - 1) // 3, minlength=jb).astype(np.uint64))
                assert joint[b, r, p, -1] == (~both).sum()
            assert not (joint[b, r, 1, :-1].reshape(jb, jb) * (1 - np.eye(jb, dtype=np.uint64))).any()      # (k, k): the diagonal


def _block(rng, dtype, B=2, nz=3, ny=5, nx=9, dims=3):
    shape = (B, dims) + ((nz,) if dims == 3 else ()) + (ny, nx)
    vel = (rng.standard_normal(shape) * 1.5).astype(dtype)
    p = rng.standard_normal((B, 1) + shape[2:]).astype(dtype)
    T = rng.uniform(0, 1, (B, 1) + shape[2:]).astype(dtype)
    return vel, p, T


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dims", (2, 3))
def test_host_recorder_against_the_checker(dtype, dims):
    rng = np.random.default_rng(11)
    channels = ("u", "v", "w", "p", "T") if dims == 3 else ("u", "v", "p", "T")
    rows = [0, 2, 4]
    ranges = {c: (-2.0, 2.0) for c in channels}
    ranges["u"] = np.array([[-2.0, 2.0], [-1.0, 3.0], [-0.5, 0.75]])                     # per listed row
    ranges["T"] = (0.1, 0.9)
    joint = (("u", "v"), ("v", "T"), ("p", "p"))
    acc = HostPlaneHistograms(channels, ranges, bins=24, joint=joint, joint_bins=8, rows=rows)
    want_c = want_j = 0
    for _ in range(3):
        vel, p, T = _block(rng, dtype, dims=dims)
        vel[1, 0, ..., 2, 3] = np.nan
        acc.update(vel, p, T)
        f = {"u": vel[:, 0], "v": vel[:, 1], "w": vel[:, dims - 1], "p": p[:, 0], "T": T[:, 0]}
        fields = [f[c] if dims == 3 else f[c][:, None] for c in channels]
        lo = np.stack([np.broadcast_to(ranges[c], (3, 2))[:, 0] for c in channels], axis=1)
        hi = np.stack([np.broadcast_to(ranges[c], (3, 2))[:, 1] for c in channels], axis=1)
        lo_r, scale = ref.tables(lo, hi, 24, dtype)
        c, j = ref.histogram(fields, rows, lo_r, scale, 24, [(channels.index(a), channels.index(b)) for a, b in joint], 8)
        want_c, want_j = want_c + c, want_j + j
    assert acc.n_samples == 3
    for k, ch in enumerate(channels):
        assert np.array_equal(acc.counts(ch), want_c[:, :, k, 1:25]) and np.array_equal(acc.below(ch), want_c[:, :, k, 0])
        assert np.array_equal(acc.above(ch), want_c[:, :, k, 25]) and np.array_equal(acc.nonfinite(ch), want_c[:, :, k, 26])
    nans = 3 * (3 if dims == 3 else 1)                               # one x column of row 2 of env 1, in each of the three samples
    assert acc.nonfinite("u")[1, 1] == nans and acc.nonfinite("u").sum() == nans
    for p, (a, b) in enumerate(joint):
        assert np.array_equal(acc.joint_counts(a, b), want_j[:, :, p, :-1].reshape(2, 3, 8, 8))
        assert np.array_equal(acc.joint_outside(a, b), want_j[:, :, p, -1])
    with pytest.raises(KeyError):
        acc.joint_counts("v", "u")
    # the accessors' arithmetic, row by row
    e = acc.edges("u")
    assert e.shape == (3, 25) and np.array_equal(e[:, 0], [-2.0, -1.0, -0.5]) and np.allclose(e[:, -1], [2.0, 3.0, 0.75], rtol=1e-15)
    for b in range(2):
        for r in range(3):
            c, (lo, hi) = acc.counts("u")[b, r], ranges["u"][r]
            assert np.allclose(acc.pdf("u")[b, r], ref.pdf(c, lo, hi), rtol=1e-13)
            assert np.allclose(acc.cdf("u")[b, r], ref.cdf(c), rtol=1e-13)
            assert np.isclose(acc.mean("u")[b, r], ref.mean(c, lo, hi), rtol=1e-12, atol=1e-14)
            assert np.isclose(acc.variance("u")[b, r], ref.variance(c, lo, hi), rtol=1e-12)
            for q in (0.0, 0.1, 0.5, 0.9, 1.0):
                assert np.isclose(acc.quantile("u", q)[b, r], ref.quantile(c, lo, hi, q), rtol=1e-12, atol=1e-14), q
            assert np.isclose((acc.pdf("u")[b, r] * acc.width("u")[r]).sum(), 1.0, rtol=1e-13)
            area = acc.width("u")[r] * 3 * acc.width("v")[r] * 3
            assert np.isclose(acc.joint_pdf("u", "v")[b, r].sum() * area, 1.0, rtol=1e-13)
            for hole in (0.0, 0.5):
                share, part = ref.quadrants(acc.joint_counts("u", "v")[b, r], acc.joint_centers("u")[r], acc.joint_centers("v")[r], hole=hole)
                got = acc.quadrants("u", "v", hole=hole)
                assert np.allclose(got["share"][b, r], share, rtol=1e-12, atol=1e-15)
                assert np.allclose(got["contribution"][b, r], part, rtol=1e-11, atol=1e-14)
    assert acc.quantile("u", [0.25, 0.75]).shape == (2, 3, 2)


def _hand_made():
    """One env, one row, 4 bins on [0, 4] (centres 0.5 .. 3.5) for both channels and a 4 x 4 joint table written by hand."""
    acc = HostPlaneHistograms(("u", "v"), {"u": (0.0, 4.0), "v": (0.0, 4.0)}, bins=4, joint=(("u", "v"),), joint_bins=4, rows=[0])
    acc._resolve(1, 1, 16, np.float64)
    table = np.array([[1, 0, 0, 2],
                      [0, 1, 0, 0],
                      [0, 0, 3, 0],
                      [4, 0, 0, 5]], np.uint64)
    counts = np.zeros((1, 1, 2, 7), np.uint64)
    counts[0, 0, 0, 1:5] = table.sum(axis=1)          # u: 3 1 3 9
    counts[0, 0, 1, 1:5] = table.sum(axis=0)          # v: 5 1 3 7
    joint = np.zeros((1, 1, 1, 17), np.uint64)
    joint[0, 0, 0, :16] = table.ravel()
    acc._set_state(counts, joint)
    acc.n_samples = 1
    return acc, table


def test_accessors_on_a_hand_made_table():
    acc, table = _hand_made()
    assert acc.counts("u")[0, 0].tolist() == [3, 1, 3, 9] and acc.centers("u")[0].tolist() == [0.5, 1.5, 2.5, 3.5]
    assert acc.pdf("u")[0, 0].tolist() == [3 / 16, 1 / 16, 3 / 16, 9 / 16] and acc.pdf("u").sum() == 1.0       # width 1
    assert acc.cdf("u")[0, 0].tolist() == [3 / 16, 4 / 16, 7 / 16, 1.0]
    mean_u = (3 * 0.5 + 1.5 + 3 * 2.5 + 9 * 3.5) / 16
    assert acc.mean("u")[0, 0] == mean_u == 2.625
    assert np.isclose(acc.variance("u")[0, 0], (3 * 0.25 + 2.25 + 3 * 6.25 + 9 * 12.25) / 16 - mean_u ** 2, rtol=1e-14)
    # quantiles, linear inside a bin: 3 of 16 cells below 1, 4 below 2, 7 below 3
    assert acc.quantile("u", 3 / 16)[0, 0] == 1.0 and acc.quantile("u", 0.25)[0, 0] == 2.0
    assert acc.quantile("u", 5.5 / 16)[0, 0] == 2.5 and acc.quantile("u", 0.0)[0, 0] == 0.0 and acc.quantile("u", 1.0)[0, 0] == 4.0
    assert np.isclose(acc.quantile("u", 11.5 / 16)[0, 0], 3.5)
    with pytest.raises(ValueError):
        acc.quantile("u", 1.5)
    # quadrants about (2, 2): Q1 = table[2:, 2:], Q2 = table[:2, 2:], Q3 = table[:2, :2], Q4 = table[2:, :2]
    q = acc.quadrants("u", "v", mean_a=2.0, mean_b=2.0)
    assert q["share"][0, 0].tolist() == [8 / 16, 2 / 16, 2 / 16, 4 / 16, 0.0]
    prod = lambda i, j: (i + 0.5 - 2.0) * (j + 0.5 - 2.0)
    want = [(3 * prod(2, 2) + 5 * prod(3, 3)) / 16, 2 * prod(0, 3) / 16, (prod(0, 0) + prod(1, 1)) / 16, 4 * prod(3, 0) / 16, 0.0]
    assert np.allclose(q["contribution"][0, 0], want, rtol=1e-15)
    x = np.arange(4) + 0.5
    cov = (table * np.outer(x - 2.0, x - 2.0)).sum() / 16
    assert np.isclose(q["contribution"].sum(), cov, rtol=1e-14)
    # the histogram's own means, and a hole that takes the weak cells out of the four quadrants
    own = acc.quadrants("u", "v", hole=0.6)
    share, part = ref.quadrants(table, x, x, hole=0.6)
    assert np.allclose(own["share"][0, 0], share) and np.allclose(own["contribution"][0, 0], part) and own["share"][0, 0, 4] > 0
    assert np.isclose(own["share"].sum(), 1.0)
    assert np.isclose(acc.joint_pdf("u", "v").sum(), 1.0) and acc.joint_outside("u", "v")[0, 0] == 0


def test_merge_pooled_save_load(tmp_path):
    rng = np.random.default_rng(2)
    mk = lambda **kw: HostPlaneHistograms(("u", "v", "p"), {"u": (-2, 2), "v": (-2, 2), "p": (-3, 3)}, bins=16, joint=(("u", "v"),),
                                          joint_bins=4, **kw)
    a, b, both = mk(), mk(), mk()
    s = [_block(rng, np.float32, dims=2) for _ in range(3)]
    a.update(*s[0][:2])
    b.update(*s[1][:2])
    b.update(*s[2][:2])
    for t in s:
        both.update(*t[:2])
    a.merge(b)
    assert a.n_samples == 3 and np.array_equal(a._counts, both._counts) and np.array_equal(a._joint, both._joint)
    fresh = mk().merge(b)                                            # an empty host record takes the other
    assert fresh.n_samples == 2 and np.array_equal(fresh.counts("p"), b.counts("p"))
    pooled = both.pooled()
    assert pooled.counts("u").shape == (1, 5, 16) and np.array_equal(pooled.counts("u")[0], both.counts("u").sum(axis=0))
    assert np.array_equal(pooled.joint_counts("u", "v")[0], both.joint_counts("u", "v").sum(axis=0)) and pooled.n_samples == 3
    path = str(tmp_path / "hist.npz")
    both.save(path)
    back = HostPlaneHistograms.load(path)
    assert back.n_samples == 3 and back.channels == both.channels and back.joint == both.joint and back.rows.tolist() == [0, 1, 2, 3, 4]
    assert np.array_equal(back._counts, both._counts) and np.array_equal(back._joint, both._joint) and back._counts.dtype == np.uint64
    assert np.array_equal(back.scale, both.scale) and back.scale.dtype == np.float32 and np.array_equal(back.edges("p"), both.edges("p"))
    back.merge(both)
    assert np.array_equal(back.counts("v"), 2 * both.counts("v"))
    # differing tables
    other = HostPlaneHistograms(("u", "v", "p"), {"u": (-2, 2), "v": (-2, 2), "p": (-3, 3.5)}, bins=16, joint=(("u", "v"),), joint_bins=4)
    other.update(*s[0][:2])
    with pytest.raises(ValueError, match="merge"):
        both.merge(other)
    other = HostPlaneHistograms(("u", "v", "p"), {"u": (-2, 2), "v": (-2, 2), "p": (-3, 3)}, bins=8, joint=(("u", "v"),), joint_bins=4)
    other.update(*s[0][:2])
    with pytest.raises(ValueError, match="merge"):
        both.merge(other)
    wide = mk()
    wide.update(*(t.astype(np.float64) for t in s[0][:2]))          # another dtype: another rounding of the tables
    with pytest.raises(ValueError, match="merge"):
        both.merge(wide)
    with pytest.raises(RuntimeError, match="no sample recorded yet"):
        mk().counts("u")


R2 = {"u": (-1.0, 1.0), "v": (-1.0, 1.0)}


@pytest.mark.parametrize("args,kw", [
    (((), {}), {}),                                                              # no channel
    ((("u", "q"), {"u": (0, 1), "q": (0, 1)}), {}),                              # an unknown name
    ((("v", "u"), R2), {}),                                                      # not in the order u, v, w, p, T
    ((("u", "u"), {"u": (0, 1)}), {}),
    ((("u", "v"), {"u": (-1.0, 1.0)}), {}),                                      # a channel without a range
    ((("u", "v"), {**R2, "p": (0, 1)}), {}),                                     # a range without a channel
    ((("u", "v"), {**R2, "u": (1.0, 1.0)}), {}),                                 # hi <= lo
    ((("u", "v"), {**R2, "u": (1.0, -1.0)}), {}),
    ((("u", "v"), {**R2, "u": (0.0, np.inf)}), {}),                              # a non-finite edge
    ((("u", "v"), {**R2, "u": (np.nan, 1.0)}), {}),
    ((("u", "v"), {**R2, "u": np.zeros((3, 3))}), {}),                           # a range of another shape
    ((("u", "v"), {**R2, "u": [[-1, 1], [-1, 1]]}), dict(rows=[0, 1, 2])),       # ranges per row, another number of rows
    ((("u", "v"), R2), dict(bins=1)),
    ((("u", "v"), R2), dict(bins=257)),
    ((("u", "v"), R2), dict(bins=128, joint_bins=1)),
    ((("u", "v"), R2), dict(bins=256, joint_bins=128)),
    ((("u", "v"), R2), dict(bins=12, joint_bins=8)),                             # not a divisor
    ((("u", "v"), R2), dict(joint=(("u", "p"),))),                               # a pair outside the channels
    ((("u", "v"), R2), dict(joint=(("u", "v", "u"),))),
    ((("u", "v"), R2), dict(joint=(("u", "v"), ("u", "v")))),                    # a pair twice
    ((("u", "v"), R2), dict(joint=(("u", "v"), ("v", "u"), ("u", "u"), ("v", "v"), ("u", "v"), ("v", "u"), ("u", "u")))),  # seven
    ((("u", "v"), R2), dict(rows=[])),
    ((("u", "v"), R2), dict(rows=[2, 1])),                                       # not ascending
    ((("u", "v"), R2), dict(rows=[1, 1])),
    ((("u", "v"), R2), dict(rows=[-1, 0])),
])
def test_constructor_refusals(args, kw):
    for cls in (HostPlaneHistograms, PlaneHistograms):
        with pytest.raises(ValueError):
            cls(*args, **kw)


def test_update_refusals():
    rng = np.random.default_rng(0)
    vel, p, T = _block(rng, np.float32, dims=2)
    with pytest.raises(ValueError, match="outside the grid"):
        HostPlaneHistograms(("u", "v"), R2, rows=[0, 5]).update(vel)
    with pytest.raises(ValueError, match="rows"):
        HostPlaneHistograms(("u", "v"), {**R2, "u": np.array([[-1.0, 1.0]] * 4)}).update(vel)          # 4 ranges, 5 rows
    with pytest.raises(ValueError, match="pressure"):
        HostPlaneHistograms(("u", "p"), {"u": (0, 1), "p": (0, 1)}).update(vel)
    with pytest.raises(ValueError, match="channel T"):
        HostPlaneHistograms(("u", "T"), {"u": (0, 1), "T": (0, 1)}).update(vel, p)
    with pytest.raises(ValueError, match="do not fit"):
        HostPlaneHistograms(("u", "w"), {"u": (0, 1), "w": (0, 1)}).update(vel)
    with pytest.raises(ValueError, match="do not fit float32"):
        HostPlaneHistograms(("u",), {"u": (0.0, 1e-42)}).update(vel)                                   # scale overflows the dtype
    with pytest.raises(TypeError):
        HostPlaneHistograms(("u",), {"u": (0, 1)}).update(vel.astype(np.float16))
    acc = HostPlaneHistograms(("u",), {"u": (0, 1)})
    acc.update(vel)
    with pytest.raises(ValueError, match="changed"):
        acc.update(vel.astype(np.float64))
    with pytest.raises(ValueError, match="batch size"):
        acc.update(vel[:1])
    with pytest.raises(ValueError, match="on the GPU"):
        PlaneHistograms(("u",), {"u": (0, 1)}).update(vel)
    HostPlaneHistograms(("u", "T"), {"u": (0, 1), "T": (0, 1)}).update(vel, None, T)                   # no pressure needed


# ---- the C ABI: refusals before any launch (host tables, null or dummy device pointers)

def _call(lib, f64, **over):
    a = dict(K=2, batch=3, nz=2, ny=6, nx=8, rows=[0, 2, 5], bins=16, pairs=[(0, 1)], joint_bins=4, channels="dummy", strides=None,
             lo=ctypes.c_void_p(64), scale=ctypes.c_void_p(64), counts=ctypes.c_void_p(64), joint=ctypes.c_void_p(64), rows_null=False)
    a.update(over)
    K = max(a["K"], 1)
    field = a["nz"] * a["ny"] * a["nx"]
    ptrs = None if a["channels"] is None else (ctypes.c_void_p * 5)(*([4096] * min(K, 5) + [None] * (5 - min(K, 5))))
    if a["channels"] == "null_entry":
        ptrs[0] = None
    strides = (ctypes.c_int64 * 5)(*(a["strides"] or [max(field, 1)] * 5))
    rows = None if a["rows_null"] else (ctypes.c_int32 * max(len(a["rows"]), 1))(*a["rows"])
    flat = [i for p in a["pairs"] or () for i in p]
    pairs = (ctypes.c_int32 * max(len(flat), 1))(*flat) if a["pairs"] is not None else None
    n_pairs = over.get("n_pairs", len(a["pairs"]) if a["pairs"] is not None else 1)
    return lib.fg_plane_histogram(ptrs, strides, a["K"], a["batch"], a["nz"], a["ny"], a["nx"], rows, over.get("n_rows", len(a["rows"])),
                                  a["lo"], a["scale"], a["bins"], pairs, n_pairs, a["joint_bins"], a["counts"], a["joint"], None)


INVALID = [
    dict(channels=None), dict(channels="null_entry"), dict(rows_null=True), dict(lo=None), dict(scale=None), dict(counts=None),
    dict(joint=None),                                         # joint == NULL with n_pairs = 1
    dict(pairs=[], n_pairs=0),                                # joint != NULL with n_pairs = 0
    dict(pairs=None),
    dict(K=0), dict(K=6), dict(bins=1), dict(bins=257), dict(joint_bins=1), dict(bins=256, joint_bins=128), dict(bins=12, joint_bins=8),
    dict(n_pairs=-1), dict(pairs=[(0, 1)] * 7), dict(pairs=[(0, 2)]), dict(pairs=[(-1, 0)]),
    dict(n_rows=0), dict(rows=[0, 1, 2, 3, 4, 5, 5]), dict(rows=[0, 2, 2]), dict(rows=[2, 1]), dict(rows=[0, 6]), dict(rows=[-1, 3]),
    dict(batch=0), dict(nz=0), dict(ny=0), dict(nx=-3),
    dict(strides=[95] * 5),                                   # below nz * ny * nx = 96
    dict(nz=2 ** 15 + 1, nx=2 ** 15, ny=1, rows=[0], strides=[2 ** 62] * 5),             # a plane above 2^30 cells
    dict(batch=2 ** 30, ny=4, rows=[0, 1], nz=1, nx=1, strides=[4] * 5),                 # batch * n_rows above 2^31 - 1
]


@pytest.mark.parametrize("case", range(len(INVALID)))
def test_abi_argument_errors_come_before_any_launch(case):
    for f64, lib in ((False, L.load()), (True, L.load_f64())):
        assert _call(lib, f64, **INVALID[case]) == L.FG_ERR_INVALID_ARG, INVALID[case]
        assert b"fg_plane_histogram" in lib.fg_last_error()


def test_abi_unsupported_sizes_come_before_any_launch():
    for f64, lib in ((False, L.load()), (True, L.load_f64())):
        # a plane of up to 1024 cells: four rows share the workgroup's LDS, K = 5, bins = 256, three pairs at 64 x 64 do not fit
        big = dict(K=5, bins=256, pairs=[(0, 1), (1, 2), (3, 4)], joint_bins=64)
        assert _call(lib, f64, nz=4, nx=256, **big) == L.FG_ERR_UNSUPPORTED
        assert b"LDS" in lib.fg_last_error()


def test_symbol_is_declared_typed_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fluidgym_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+fg_plane_histogram\s*\(", text)
    assert "fg_plane_histogram" in L.SIGNATURES and "fg_plane_histogram" in L.SIGNATURES_F64
    assert len(L.SIGNATURES["fg_plane_histogram"][1]) == 18
    for lib in (L.load(), L.load_f64()):
        assert hasattr(lib, "fg_plane_histogram")
    assert "fg_plane_histogram" not in open(os.path.join(ROOT, "fluidgym_amd", "csrc", "fg_f64_stubs.hip")).read()
    mk = open(os.path.join(ROOT, "fluidgym_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS = .*\bfg_planehist\.hip", mk, re.M) and re.search(r"^F64_SRCS = .*\bfg_planehist\.hip", mk, re.M)
    assert re.search(r"fg_planehist\.o \$\(F64_DIR\)/fg_planehist\.o: CXXFLAGS \+= -ffp-contract=off", mk)


def test_env_needs_a_reset_and_is_off_by_default():
    env = fluidgym_amd.make("RBC2D-easy-v0", num_envs=2, cuda_device="cpu")
    assert env._hook("flow_hist") is None
    with pytest.raises(RuntimeError, match="reset"):
        env.start_flow_histograms()
    with pytest.raises(RuntimeError, match="no histograms"):
        env.stop_flow_histograms()
