"""Shared by the cell-statistics tests: seeded flat multi-block fields (a smooth mean that drifts from sample to sample plus skewed
noise), the long-double one-shot evaluation over the concatenated samples, and the comparison in units of the absolute-monomial
sum."""
import numpy as np

BOUND_GOLDEN = 1e-13      # against the reference's accumulators and between the twins: x the absolute-monomial sum
BOUND_ONE_SHOT = 1e-11    # against the long-double one-shot: x the absolute-monomial sum


def layout(sizes):
    """``(size, cell_offset)`` per block for blocks packed one after the other, and the number of cells."""
    blocks, off = [], 0
    for size in sizes:
        blocks.append((tuple(size), off))
        off += int(np.prod(size))
    return blocks, off


def make_fields(sizes, B, samples=3, seed=0, dtype=np.float32):
    """``samples`` x (velocity [B, d, N], pressure [B, N]) for blocks of ``sizes`` = (nx, ny[, nz]) each."""
    d = len(sizes[0])
    _, N = layout(sizes)
    rng = np.random.default_rng(seed)
    smooth = np.cos(np.linspace(0.0, 7.0, N))
    out = []
    for s in range(samples):
        u = rng.standard_normal((B, d, N))
        u = 0.3 * u + 0.1 * u ** 2 + 0.2 * s
        u[:, 0] += 1.0 + smooth
        p = 0.5 - 0.3 * s - smooth + 0.2 * rng.standard_normal((B, N)) ** 3
        out.append((u.astype(dtype), p.astype(dtype)))
    return out


def one_shot(rec, fields, pool_envs=False):
    """Long-double evaluation over the concatenated samples ``fields`` for the layout of the record ``rec``: n [NC],
    mean [B, K, NC], central [B, P, NC] and the absolute-monomial sums abs1 [B, K, NC] (of |x|), absM [B, P, NC] (of |d_i d_j|)."""
    v = np.stack([np.concatenate([np.moveaxis(np.asarray(u), 1, 0), np.asarray(p)[None]]) for u, p in fields]).astype(np.longdouble)
    S, K, B, _ = v.shape                                                         # [S, K, B, N]
    if pool_envs:
        v = np.moveaxis(v, 2, 0).reshape(S * B, K, 1, -1)
    ns, means, cens, abs1, absM = [], [], [], [], []
    for off, layer, nz, _ in rec.table:
        c = v[..., off:off + nz * layer].reshape(v.shape[:3] + (nz, layer))
        c = np.moveaxis(c, 0, 2).reshape(K, v.shape[2], -1, layer)               # [K, B, cells of a column, layer]
        n = c.shape[2]
        m = c.sum(axis=2) / n
        d = c - m[:, :, None]
        ns.append(np.full(layer, float(n)))
        means.append(m)
        abs1.append(np.abs(c).sum(axis=2))
        cens.append(np.stack([(d[i] * d[j]).sum(axis=1) for i, j in rec.pairs]))
        absM.append(np.stack([np.abs(d[i] * d[j]).sum(axis=1) for i, j in rec.pairs]))
    cat = lambda parts: np.moveaxis(np.concatenate(parts, axis=-1), 0, 1)
    return np.concatenate(ns), cat(means), cat(cens), cat(abs1), cat(absM)


def worst_errors(rec, truth):
    """(mean error / (abs1 / n), central error / absM), each the maximum over the record; n must be exact."""
    n, mean, cen, abs1, absM = truth
    gm, gc = rec._state()
    assert np.array_equal(rec.flat("n")[0], n), (rec.flat("n")[0], n)
    assert gm.shape == mean.shape and gc.shape == cen.shape, (gm.shape, mean.shape, gc.shape, cen.shape)
    em = np.abs(gm.astype(np.longdouble) - mean) / (abs1 / n)
    ec = np.abs(gc.astype(np.longdouble) - cen)
    ec = np.where(absM > 0, ec / np.where(absM > 0, absM, 1), np.where(ec == 0, 0, np.inf))      # one cell: exactly 0
    return float(em.max()), float(ec.max())
