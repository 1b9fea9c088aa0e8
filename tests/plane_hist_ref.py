"""The checker of the plane histograms, in NumPy: the bin rule in the field's dtype with the subtraction and the multiplication as
two operations, the joint rule, and the arithmetic of the accessors -- written cell by cell and bin by bin, apart from
``fluidgym_amd.simulation.plane_hist``."""
import numpy as np


def tables(lo, hi, bins, dtype):
    """``lo``, ``hi`` fp64 (any shape) -> the rounded ``lo`` and ``scale = bins / (hi - lo)`` (formed in fp64, rounded once)."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    return lo.astype(dtype), (np.float64(bins) / (hi - lo)).astype(dtype)


def slots(v, lo, scale, bins):
    """Slot of every element of ``v`` (one dtype with the scalars ``lo`` and ``scale``)."""
    dt = v.dtype.type
    lo, scale = dt(lo), dt(scale)
    assert type(lo) is dt and type(scale) is dt
    out = np.empty(v.shape, np.int64)
    flat, o = v.reshape(-1), out.reshape(-1)
    with np.errstate(all="ignore"):
        d = flat - lo                         # one rounding
        t = d * scale                         # another
    assert d.dtype == v.dtype and t.dtype == v.dtype
    for i in range(flat.size):
        if flat[i] != flat[i]:
            o[i] = bins + 2
        elif not (t[i] >= dt(0)):
            o[i] = 0
        elif t[i] >= dt(bins):
            o[i] = bins + 1
        else:
            o[i] = 1 + int(t[i])
    return out


def histogram(fields, rows, lo, scale, bins, pairs=(), joint_bins=2):
    """``fields``: K arrays ``[B, nz, ny, nx]``; ``lo``, ``scale`` ``[R, K]`` in the fields' dtype -> ``counts [B, R, K, bins + 3]``,
    ``joint [B, R, P, joint_bins^2 + 1]`` (``uint64``) of one sample."""
    K, (B, nz, ny, nx) = len(fields), fields[0].shape
    R, P, ratio, J = len(rows), len(pairs), bins // joint_bins, joint_bins * joint_bins
    assert bins % joint_bins == 0
    counts = np.zeros((B, R, K, bins + 3), np.uint64)
    joint = np.zeros((B, R, P, J + 1), np.uint64)
    for b in range(B):
        for r, y in enumerate(rows):
            s = [slots(np.ascontiguousarray(fields[k][b, :, y, :]), lo[r, k], scale[r, k], bins).reshape(-1) for k in range(K)]
            for k in range(K):
                np.add.at(counts[b, r, k], s[k], np.uint64(1))
            for p, (ia, ib) in enumerate(pairs):
                for sa, sb in zip(s[ia], s[ib]):
                    if 1 <= sa <= bins and 1 <= sb <= bins:
                        joint[b, r, p, (sa - 1) // ratio * joint_bins + (sb - 1) // ratio] += np.uint64(1)
                    else:
                        joint[b, r, p, J] += np.uint64(1)
    return counts, joint


# ---- the accessors' arithmetic, for one row: c = counts of the bins [bins], lo / hi the row's range

def edges(lo, hi, bins):
    return np.array([lo + (hi - lo) * (i / bins) for i in range(bins + 1)])


def centers(lo, hi, bins):
    e = edges(lo, hi, bins)
    return np.array([0.5 * (e[i] + e[i + 1]) for i in range(bins)])


def pdf(c, lo, hi):
    c = np.asarray(c, np.float64)
    return c / (c.sum() * ((hi - lo) / len(c)))


def cdf(c):
    c = np.asarray(c, np.float64)
    return np.array([c[:i + 1].sum() for i in range(len(c))]) / c.sum()


def quantile(c, lo, hi, q):
    """Linear inside the first bin whose cumulative count reaches ``q`` times the total."""
    c = np.asarray(c, np.float64)
    e, target, before = edges(lo, hi, len(c)), q * c.sum(), 0.0
    for i in range(len(c)):
        if before + c[i] >= target or i == len(c) - 1:
            return e[i] + (e[i + 1] - e[i]) * ((target - before) / c[i] if c[i] > 0 else 0.0)
        before += c[i]


def mean(c, lo, hi):
    c = np.asarray(c, np.float64)
    return float((c * centers(lo, hi, len(c))).sum() / c.sum())


def variance(c, lo, hi):
    c = np.asarray(c, np.float64)
    x = centers(lo, hi, len(c))
    return float((c * (x - mean(c, lo, hi)) ** 2).sum() / c.sum())


def quadrants(table, xa, xb, mean_a=None, mean_b=None, hole=0.0):
    """``table [jb, jb]`` with bin centres ``xa``, ``xb`` -> (share [5], contribution [5]) for Q1..Q4 and the hole."""
    t = np.asarray(table, np.float64)
    n = t.sum()
    ma = (t.sum(axis=1) * xa).sum() / n if mean_a is None else mean_a
    mb = (t.sum(axis=0) * xb).sum() / n if mean_b is None else mean_b
    rms_a = np.sqrt((t.sum(axis=1) * (xa - ma) ** 2).sum() / n)
    rms_b = np.sqrt((t.sum(axis=0) * (xb - mb) ** 2).sum() / n)
    share, part = np.zeros(5), np.zeros(5)
    for i in range(t.shape[0]):
        for j in range(t.shape[1]):
            da, db = xa[i] - ma, xb[j] - mb
            if abs(da * db) <= hole * rms_a * rms_b:
                q = 4
            elif da > 0:
                q = 0 if db > 0 else 3
            else:
                q = 1 if db > 0 else 2
            share[q] += t[i, j] / n
            part[q] += t[i, j] * da * db / n
    return share, part
