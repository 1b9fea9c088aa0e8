"""Shared by the budget tests: seeded samples on a grid with a non-uniform y, the long-double one-shot evaluation over the
concatenated samples of all ``K`` means and ``M`` central sums (the gradients formed from the inputs as they were cast, both border
modes), and the comparison in units of the absolute-monomial sum.  The bounds are those of ``tests/plane_stats_ref.py``."""
import numpy as np

from fluidgym_amd.simulation.plane_budgets import budget_keys
from tests.plane_stats_ref import BOUND_GOLDEN, BOUND_ONE_SHOT  # noqa: F401

LD = np.longdouble


def make_grid(nz, ny, nx):
    """Cell centres: uniform x and z, tanh-refined y between walls at -1 and 1 (symmetric about 0)."""
    e = np.tanh(1.7 * np.linspace(-1.0, 1.0, ny + 1)) / np.tanh(1.7)
    return (np.arange(nx) + 0.5) * 0.37, 0.5 * (e[1:] + e[:-1]), (np.arange(nz) + 0.5) * 0.21


def make_samples(shape, samples=3, seed=0, dtype=np.float32):
    """``samples`` x (velocity [B, 3, Z, Y, X], pressure [B, 1, Z, Y, X], source [B, 3, Z, Y, X]) for ``shape = (B, nz, ny, nx)``: a
    mean profile sheared in y that drifts from sample to sample, skewed fluctuations."""
    B, nz, ny, nx = shape
    rng = np.random.default_rng(seed)
    prof = np.linspace(0.2, 1.7, ny).reshape((ny, 1))
    out = []
    for s in range(samples):
        u = rng.standard_normal((B, 3, nz, ny, nx))
        u = 0.3 * u + 0.1 * u ** 2 + 0.2 * s
        u[:, 0] += prof
        p = 0.5 - 0.3 * s + 0.2 * rng.standard_normal((B, 1, nz, ny, nx)) ** 3
        f = 0.1 * s + 0.2 * rng.standard_normal((B, 3, nz, ny, nx))
        f[:, 0] += 0.5 * prof
        out.append(tuple(a.astype(dtype) for a in (u, p, f)))
    return out


def _gradient(f, pos, axis, wrap):
    pos = np.asarray(pos, np.float64).astype(LD)          # the ghost positions as the code forms them, then exact arithmetic
    g = np.concatenate([[2 * pos[0] - pos[1]], pos, [2 * pos[-1] - pos[-2]]])
    lo, hi = np.roll(f, 1, axis), np.roll(f, -1, axis)
    if not wrap:
        first, last = [slice(None)] * f.ndim, [slice(None)] * f.ndim
        first[axis], last[axis] = slice(0, 1), slice(f.shape[axis] - 1, None)
        lo[tuple(first)] = 0
        hi[tuple(last)] = 0
    shape = [1] * f.ndim
    shape[axis] = -1
    return (hi - lo) / np.abs(g[2:] - g[:-2]).reshape(shape)


def channel_stack(sample, grid, forcing, wrap):
    """[K, B, nz, ny, nx] long double of one sample: the values as they were cast, the gradients in long double."""
    u, p, s = sample
    x, y, z = grid
    f = [np.asarray(u[:, c]).astype(LD) for c in range(3)] + [np.asarray(p[:, 0]).astype(LD)]
    axes = ((x, 3, wrap[0]), (y, 2, False), (z, 1, wrap[1]))
    ch = f[:3] + [_gradient(f[3], pos, ax, w) for pos, ax, w in axes]
    for pos, ax, w in axes:
        ch += [_gradient(f[i], pos, ax, w) for i in range(3)]
    if forcing:
        ch += [np.asarray(s[:, c]).astype(LD) for c in range(3)]
    return np.stack(ch)


def one_shot(stacks, forcing, pool_envs=False):
    """Long-double evaluation over the concatenated samples ``stacks`` (each [K, B, nz, ny, nx]): n [B], mean [B, ny, K],
    central [B, ny, M] and the absolute-monomial sums abs1 [B, ny, K] (of |x|), absM [B, ny, M] (of |prod d|)."""
    v = np.concatenate([np.asarray(s, LD) for s in stacks], axis=2)       # along z: all cells of a row
    if pool_envs:
        v = np.concatenate([v[:, b:b + 1] for b in range(v.shape[1])], axis=2)
    n = v.shape[2] * v.shape[4]
    mean = v.sum(axis=(2, 4)) / n
    d = v - mean[:, :, None, :, None]
    cen, absM = [], []
    for key in budget_keys(forcing):
        m = np.prod([d[c] for c in key], axis=0)
        cen.append(m.sum(axis=(1, 3)))
        absM.append(np.abs(m).sum(axis=(1, 3)))
    to = lambda a: np.moveaxis(np.asarray(a), 0, -1)
    return (np.full(v.shape[1], float(n)), to(mean), to(cen), to(np.abs(v).sum(axis=(2, 4))), to(absM))


def scaled_errors(state, truth):
    """(mean error / (abs1 / n), central error / absM) per element for a state (n, mean, central); n must be exact."""
    n, mean, cen, abs1, absM = truth
    gn, gm, gc = state
    assert np.array_equal(gn, n), (gn, n)
    em = np.abs(np.asarray(gm).astype(LD) - mean)                     # (a channel that is 0 in every cell -- d/dx on a wrapped
    em = np.where(abs1 > 0, em / np.where(abs1 > 0, abs1 / n[:, None, None], 1), np.where(em == 0, 0, np.inf))   # axis of two cells)
    ec = np.abs(np.asarray(gc).astype(LD) - cen)
    ec = np.where(absM > 0, ec / np.where(absM > 0, absM, 1), np.where(ec == 0, 0, np.inf))
    return em, ec


def worst_errors(rec, truth, keys=None):
    """The maxima of ``scaled_errors`` over the record; ``keys``: a boolean mask over the central sums to look at."""
    em, ec = scaled_errors(rec._state(), truth)
    if keys is not None:
        ec = ec[..., np.asarray(keys)]
    return float(em.max()), float(ec.max())
