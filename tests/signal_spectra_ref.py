"""What the signal-spectra tests share: the seeded series, SciPy's Welch estimates of it and the error measure."""
import numpy as np

DETRENDS = ("none", "constant", "linear")
SCIPY_DETREND = {"none": False, "constant": "constant", "linear": "linear"}


def three_signals(L: int, seed: int = 0, dtype=np.float64) -> np.ndarray:
    """``[5 L + 7, 3]``: a mean of 3.2 plus a sine plus noise, a phase-shifted sine plus a drift, white noise."""
    n = 5 * L + 7
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    f0 = 3.3 / L * 2.0 * np.pi                                  # between bins 3 and 4
    a = 3.2 + np.sin(f0 * t) + 0.1 * rng.standard_normal(n)
    b = 0.7 * np.sin(f0 * t + 0.9) + 0.004 * t
    c = rng.standard_normal(n)
    return np.stack([a, b, c], axis=1).astype(dtype)


def batch_series(B: int, widths, L: int, seed: int = 0, dtype=np.float64) -> np.ndarray:
    """``[5 L + 7, B, S]`` with ``S = sum(widths)``: per env and signal an offset, a sine of its own frequency and phase, a drift
    and noise."""
    n, S = 5 * L + 7, int(sum(widths))
    rng = np.random.default_rng([seed, B, S, L])
    t = np.arange(n)[:, None, None]
    freq = (1.5 + 5.0 * rng.random((1, B, S))) / L * 2.0 * np.pi
    x = rng.normal(0.0, 2.0, (1, B, S)) + np.sin(freq * t + rng.random((1, B, S)) * 6.0) + 0.01 * rng.random((1, B, S)) * t
    return (x + 0.3 * rng.standard_normal((n, B, S))).astype(dtype)


def scipy_welch(x, y, L, noverlap, window, detrend, dt):
    """``scipy.signal.welch`` (``y`` None) or ``csd`` of 1-D series, ``average="mean"``, ``scaling="density"``."""
    from scipy import signal

    kw = dict(fs=1.0 / dt, window=window, nperseg=L, noverlap=noverlap, detrend=SCIPY_DETREND[detrend], scaling="density",
              average="mean", return_onesided=True)
    return (signal.welch(x, **kw) if y is None else signal.csd(x, y, **kw))[1]


def n_segments(n: int, L: int, noverlap: int) -> int:
    return 0 if n < L else 1 + (n - L) // (L - noverlap)


def rel_max(got, want) -> float:
    """``max |got - want| / max |want|``; inf when ``got`` is not finite where ``want`` is."""
    got, want = np.asarray(got), np.asarray(want)
    if not np.isfinite(got).all():
        return float("inf")
    return float(np.abs(got - want).max() / np.abs(want).max())
