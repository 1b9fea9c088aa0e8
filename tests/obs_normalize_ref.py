"""NumPy fp64 checker of the running normalisation (``fluidgym_amd/csrc/fg_obsnorm.hip``, ``fluidgym_amd/wrappers/normalize.py``;
DESIGN.md section 6o): two-pass batch moments, the merge, the normalisation and the return update, restated from the contract.  It sums
in NumPy's own order, so the kernels are compared with it by derived bounds, not bit for bit.

The bounds (``tolerances``), with u = 2^-53 and data |x| <= 8:

* a sum of k values in ANY order is within (k - 1) u sum|x| of the exact sum, so a batch mean of m values is within (m + 1) u 8 of the
  exact one; a merge adds four roundings of quantities of at most 16.  Over the life of a record of N values in at most N batches the
  kernel's mean and the checker's are each within (N + 5 N) u 8 of the exact mean of the exact arithmetic, hence within
  12 N u 8 < C N 2^-52 8 of each other with C = 8.
* the error delta of mean_b enters M2_b = sum (x - mean_b)^2 only as m delta^2, because sum (x - mu) = 0; every term is at most
  16^2 = 4 * 64 with three roundings, and the sum of m of them in any order adds (m - 1) u sum d^2: M2_b is within
  (m + 3) u 4 (64 m) of the exact value on either side, the merge term delta^2 n_a m / n <= 256 N adds five roundings.  Kernel and
  checker are within 2 (N + 8) u 256 N <= C N 2^-52 (64 N) of each other with the same C = 8.
* an fp32 output is one rounding of the fp64 value: 2^-23 max(1, |ref|) covers it and a flip of that rounding.
* an fp64 output y = (x - mean) rstd moves by rstd dmean + |y| rstd^2 dvar / 2 with dvar = dM2 / N, plus four roundings of y:
  with rstd <= RSTD_MAX = 4 (per-slot standard deviation of at least 0.25).
"""
import numpy as np

C = 8.0
X_MAX = 8.0
RSTD_MAX = 4.0


def batch_moments(x, axis=0):
    """(m, mean_b, M2_b) of the values of ``x`` along ``axis`` (``None``: all of them), two passes in fp64."""
    x = np.asarray(x, np.float64)
    m = x.shape[axis] if axis is not None else x.size
    mean = x.sum(axis=axis) / m
    d = x - (mean if axis is None else np.expand_dims(mean, axis))
    return m, mean, (d * d).sum(axis=axis)


def merge(n_a, mean_a, m2_a, m, mean_b, m2_b):
    """The record (n_a, mean_a, M2_a) advanced by a batch (m, mean_b, M2_b); an empty record gives the batch."""
    mean_b, m2_b = np.asarray(mean_b, np.float64), np.asarray(m2_b, np.float64)
    if n_a == 0:
        return m, mean_b.copy(), m2_b.copy()
    n = n_a + m
    delta = mean_b - mean_a
    return n, mean_a + delta * (m / n), m2_a + m2_b + delta * delta * (n_a * m / n)


def normalise(x, n, mean, m2, epsilon=1e-8, clip=None, dtype=None):
    """y = (x - mean) / sqrt(M2 / n + epsilon) in fp64, clipped, rounded once to ``dtype`` (default: that of x)."""
    dtype = np.asarray(x).dtype if dtype is None else dtype
    y = (np.asarray(x, np.float64) - mean) * (1.0 / np.sqrt(m2 / n + epsilon))
    if clip:
        y = np.clip(y, -clip, clip)
    return y.astype(dtype)


class Record:
    """The record of one key: ``update(x, rows)`` merges the rows ``rows`` (default all) of ``x [rows, D]``; ``pooled`` keeps one
    scalar slot whose count is rows x D."""

    def __init__(self, pooled=False):
        self.pooled, self.n, self.mean, self.m2 = pooled, 0, None, None

    def update(self, x, rows=None):
        x = np.asarray(x, np.float64)
        sel = x if rows is None else x[np.asarray(rows)]
        m, mean_b, m2_b = batch_moments(sel, axis=None if self.pooled else 0)
        self.n, self.mean, self.m2 = merge(self.n, self.mean, self.m2, m, mean_b, m2_b)
        return self

    def apply(self, x, epsilon=1e-8, clip=None):
        return normalise(x, self.n, self.mean, self.m2, epsilon, clip)


class ReturnRecord:
    """The discounted returns G and their scalar record; ``step(reward)`` returns the scaled rewards."""

    def __init__(self, rows, gamma):
        self.G, self.gamma, self.rec = np.zeros(rows, np.float64), gamma, Record(pooled=True)

    def step(self, reward, epsilon=1e-8, clip=None, update=True):
        reward = np.asarray(reward)
        self.G = self.gamma * self.G + reward.astype(np.float64).reshape(-1)
        if update:
            self.rec.update(self.G[:, None])
        y = reward.astype(np.float64) * (1.0 / np.sqrt(self.rec.m2 / self.rec.n + epsilon))
        if clip:
            y = np.clip(y, -clip, clip)
        return y.astype(reward.dtype)


def tolerances(n_values, x_max=X_MAX):
    """(bound on |mean - ref|, bound on |M2 - ref|) of a record of ``n_values`` values of magnitude up to ``x_max`` (module docstring)."""
    e = C * n_values * 2.0 ** -52
    return e * x_max, e * (x_max * x_max * n_values)


def output_tolerance(ref, n_values, dtype, x_max=X_MAX):
    """The bound on |y - ref| per element for outputs of ``dtype`` (module docstring)."""
    ref = np.abs(np.asarray(ref, np.float64))
    if np.dtype(dtype) == np.float32:
        return 2.0 ** -23 * np.maximum(1.0, ref)
    t_mean, t_m2 = tolerances(n_values, x_max)
    return RSTD_MAX * t_mean + ref * (RSTD_MAX ** 2 / 2.0) * (t_m2 / n_values) + 4.0 * 2.0 ** -52 * ref
