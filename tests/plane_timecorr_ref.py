"""Shared by the temporal-correlation tests: seeded samples with a decaying common field, and the brute-force evaluation over
every (base, lag) pair of a schedule -- no ring, no slots, one pair at a time."""
import numpy as np


def make_series(shape, channels, samples, seed=0, dtype=np.float32, decay=0.8):
    """``samples`` x (velocity [B, d, (Z,) Y, X], pressure [B, 1, ...], scalar [B, 1, ...]) for ``shape = (B, nz, ny, nx)``: a mean
    sheared in y, a common random field decaying by ``decay`` per sample, fresh noise of 0.1.  2-D when ``w`` is no channel."""
    B, nz, ny, nx = shape
    d = 3 if "w" in channels else 2
    sp = (ny, nx) if d == 2 else (nz, ny, nx)
    assert d == 3 or nz == 1
    rng = np.random.default_rng(seed)
    prof = np.linspace(0.2, 1.7, ny).reshape((ny, 1))
    common = [0.3 * rng.standard_normal((B, c) + sp) for c in (d, 1, 1)]
    out = []
    for s in range(samples):
        f = [decay ** s * c + 0.1 * rng.standard_normal(c.shape) for c in common]
        f[0][:, 0] += prof
        f[1] += 0.5
        out.append(tuple(a.astype(dtype) for a in f))
    return out


def channel_stack(sample, channels):
    """[B, K, nz, ny, nx] float64 of one sample."""
    u, p, T = sample
    src = {"u": u[:, 0], "v": u[:, 1], "w": u[:, 2] if u.shape[1] > 2 else None, "p": p[:, 0], "T": T[:, 0]}
    v = np.stack([src[c] for c in channels], axis=1).astype(np.float64)
    return v[:, :, None] if v.ndim == 4 else v


def brute_force(stacks, times, lags, stride, base_dtype=np.float64):
    """Every pair (base s0, sample s0 + lag) of the schedule, one at a time: ``acc [B, ny, K, lags, 4]`` (sums of the coefficient,
    of mean(b' c'), mean(b'^2), mean(c'^2)), ``count [lags]``, ``time_sum [B, lags]``.  ``stacks``: [B, K, nz, ny, nx] per sample;
    ``times``: [B] per sample; a base is rounded to ``base_dtype``."""
    n = len(stacks)
    B, K, nz, ny, nx = stacks[0].shape
    fluct = [np.asarray(v, np.float64) - np.asarray(v, np.float64).mean(axis=(2, 4), keepdims=True) for v in stacks]
    acc, count, time_sum = np.zeros((B, ny, K, lags, 4)), np.zeros(lags), np.zeros((B, lags))
    starts = [0] if stride is None else range(0, n, stride)
    with np.errstate(all="ignore"):
        for s0 in starts:
            b = fluct[s0].astype(base_dtype).astype(np.float64)
            bb = (b * b).mean(axis=(2, 4))                                        # [B, K, ny]
            for lag in range(lags):
                if s0 + lag >= n:
                    break
                c = fluct[s0 + lag]
                cross, cc = (b * c).mean(axis=(2, 4)), (c * c).mean(axis=(2, 4))
                for q, val in enumerate((cross / (np.sqrt(bb) * np.sqrt(cc)), cross, bb, cc)):
                    acc[..., lag, q] += np.moveaxis(val, 1, 2)
                count[lag] += 1
                time_sum[:, lag] += np.asarray(times[s0 + lag]) - np.asarray(times[s0])
    return acc, count, time_sum
