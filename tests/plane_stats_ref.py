"""Shared by the plane-statistics tests: seeded samples with a sheared mean profile, the long-double one-shot evaluation over the
concatenated samples (the yardstick for every order), and the comparison in units of the absolute-monomial sum."""
import numpy as np

from fluidgym_amd.simulation.plane_stats import moment_keys

BOUND_GOLDEN = 1e-13      # order <= 2 against the reference's values: x the absolute-monomial sum
BOUND_ONE_SHOT = 1e-11    # every order against the long-double one-shot: x the absolute-monomial sum


def make_samples(shape, K, samples=3, seed=0, dtype=np.float32):
    """``samples`` x (velocity [B, d, (Z,) Y, X], pressure [B, 1, ...], scalar [B, 1, ...] or None) for ``shape = (B, nz, ny, nx)``:
    a mean profile sheared in y that drifts from sample to sample, skewed fluctuations.  K = 3: 2-D u, v, p; 4: 3-D; 5: 3-D + T."""
    B, nz, ny, nx = shape
    d = 2 if K == 3 else 3
    sp = (ny, nx) if d == 2 else (nz, ny, nx)
    assert d == 3 or nz == 1
    rng = np.random.default_rng(seed)
    prof = np.linspace(0.2, 1.7, ny).reshape((ny, 1))
    out = []
    for s in range(samples):
        u = rng.standard_normal((B, d) + sp)
        u = 0.3 * u + 0.1 * u ** 2 + 0.2 * s
        u[:, 0] += prof
        p = 0.5 - 0.3 * s + 0.2 * rng.standard_normal((B, 1) + sp) ** 3
        T = (0.5 + 0.1 * s + 0.1 * rng.standard_normal((B, 1) + sp)) if K == 5 else None
        out.append(tuple(None if f is None else f.astype(dtype) for f in (u, p, T)))
    return out


def channel_stack(sample, K):
    """[K, B, nz, ny, nx] float64 of one sample."""
    u, p, T = sample
    f = [u[:, c] for c in range(u.shape[1])] + [p[:, 0]] + ([T[:, 0]] if K == 5 else [])
    v = np.stack(f).astype(np.float64)
    return v[:, :, None] if v.ndim == 4 else v


def one_shot(stacks, order, pool_envs=False):
    """Long-double evaluation over the concatenated samples ``stacks`` (each [K, B, nz, ny, nx]): n [B], mean [B, ny, K],
    central [B, ny, M] and the absolute-monomial sums abs1 [B, ny, K] (of |x|), absM [B, ny, M] (of |prod d^e|)."""
    v = np.concatenate([np.asarray(s, np.longdouble) for s in stacks], axis=2)       # along z: all cells of a row
    if pool_envs:
        v = np.concatenate([v[:, b:b + 1] for b in range(v.shape[1])], axis=2)
    K = v.shape[0]
    n = v.shape[2] * v.shape[4]
    mean = v.sum(axis=(2, 4)) / n
    d = v - mean[:, :, None, :, None]
    cen, absM = [], []
    for key in moment_keys(K, order):
        m = np.prod([d[c] ** e for c, e in enumerate(key) if e], axis=0)
        cen.append(m.sum(axis=(1, 3)))
        absM.append(np.abs(m).sum(axis=(1, 3)))
    to = lambda a: np.moveaxis(np.asarray(a), 0, -1)
    return (np.full(v.shape[1], float(n)), to(mean), to(cen), to(np.abs(v).sum(axis=(2, 4))), to(absM))


def worst_errors(rec, truth):
    """(mean error / (abs1 / n), central error / absM), each the maximum over the record; n must be exact."""
    n, mean, cen, abs1, absM = truth
    gn, gm, gc = rec._state()
    assert np.array_equal(gn, n), (gn, n)
    em = np.abs(gm.astype(np.longdouble) - mean) / (abs1 / n[:, None, None])
    ec = np.abs(gc.astype(np.longdouble) - cen)
    ec = np.where(absM > 0, ec / np.where(absM > 0, absM, 1), np.where(ec == 0, 0, np.inf))      # a constant plane: exactly 0
    return float(em.max()), float(ec.max())
