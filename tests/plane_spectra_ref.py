"""Shared by the plane-spectra tests: the direct one-shot ``numpy.fft.fftn`` evaluation of the sums a record holds, and the derived
error bounds.

Bounds (Higham, Accuracy and Stability of Numerical Algorithms, Thm 24.2, twiddle error <= eps): the computed transform of a slab
obeys ``||err||_2 <= 8 eps log2(nz nx) ||u^||_2``.  An element of ``amp`` is a sum over the samples of moduli, each of which can be
off by no more than its slab's ``||err||_2``; an element of ``power`` by ``2 |u^| |err| + |err|^2 <= 17 eps log2(nz nx) ||u^||_2^2``
(16 from the cross term, the rest covers the square and the fp64 accumulation)."""
import numpy as np

from tests.plane_stats_ref import channel_stack, make_samples  # noqa: F401  (re-exported: the same seeded samples)

BOUND_GOLDEN = 1e-13      # host twin against the reference's values: x the largest amplitude (both sides fp64 pocket-FFT arithmetic)


def direct_sums(stacks, table):
    """``stacks``: per sample ``[K, B, nz, ny, nx]`` -> the sums over the samples of ``|u^|`` and ``|u^|^2`` ``[B, K, T, nkz, nkx]``
    and of ``||u^||_2``, ``||u^||_2^2`` over the whole slab transform ``[B, K, T]``, in fp64."""
    amp = power = norm = norm2 = 0.0
    for s in stacks:
        v = np.moveaxis(np.asarray(s, np.float64), 0, 1)[:, :, :, table]            # [B, K, nz, T, nx]
        full = np.fft.fftn(np.moveaxis(v, 3, 2), axes=(3, 4))                        # [B, K, T, nz, nx]
        nz, nx = full.shape[-2:]
        cut = full[..., :max(nz // 2, 1), :nx // 2]
        amp = amp + np.abs(cut)
        power = power + cut.real ** 2 + cut.imag ** 2
        e2 = (full.real ** 2 + full.imag ** 2).sum(axis=(3, 4))
        norm, norm2 = norm + np.sqrt(e2), norm2 + e2
    return amp, power, norm, norm2


def bound_ratios(amp, power, truth, eps, nz, nx):
    """Worst |error| / bound of ``amp`` and of ``power`` against ``direct_sums``' ``truth``."""
    t_amp, t_power, norm, norm2 = truth
    lg = np.log2(nz * nx)
    ra = np.abs(amp - t_amp) / (8 * eps * lg * norm)[..., None, None]
    rp = np.abs(power - t_power) / (17 * eps * lg * norm2)[..., None, None]
    return float(ra.max()), float(rp.max())
