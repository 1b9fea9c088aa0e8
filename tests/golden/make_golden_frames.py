"""Writes ``tests/golden/reference_frames.npz``: what matplotlib itself gives for seeded float32 inputs, the fixture that holds
``tests/frames_ref.py`` (and through it ``fg_frame_colorize``) to the reference's colour mapping byte for byte.

For every case ``i``: ``input_i`` float32 ``[H, W]``, ``range_i`` float64 ``(vmin, vmax)`` (NaN, NaN: taken from the data, as the
reference's ``_format_render_data`` does with ``v_min = v_max = None``), ``cmap_i`` the map's name and
``frame_i = colormaps[name](clip((d - vmin) / (vmax - vmin), 0, 1), bytes=True)[..., :3]``.  ``table_<name>`` are the maps' 256 entries.
The inputs hold NaN, both infinities, every tie ``(d - vmin) / (vmax - vmin) == k / 256``, a value just below ``vmin``, ``vmin`` and
``vmax`` themselves, and a constant frame with the range taken from the data (span 0).

    python tests/golden/make_golden_frames.py        (needs matplotlib; made with 3.10.8, NumPy 2.2)
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
RANGES = [(-10, 10), (0, 1.0), (-2.5, 1.75)]
CMAPS = ["viridis", "rainbow"]


def special_input(rng, lo, hi):
    """[9, 31]: the 257 ties, the non-finite values, the ends of the range, and seeded values around the range."""
    span = float(hi) - float(lo)
    d = rng.uniform(lo - 0.2 * span, hi + 0.2 * span, size=9 * 31).astype(np.float32)
    k = np.arange(257, dtype=np.float64)
    d[:257] = (lo + span * k / 256.0).astype(np.float32)          # exact in float32 for these ranges
    d[257:263] = [np.nan, np.inf, -np.inf, np.nextafter(np.float32(lo), np.float32(-np.inf)), np.float32(hi), np.float32(lo)]
    return d.reshape(9, 31)


def main() -> None:
    import matplotlib

    rng = np.random.default_rng(20260)
    out, i = {}, 0
    for name in CMAPS:
        cmap = matplotlib.colormaps[name]
        out[f"table_{name}"] = cmap((np.arange(256) + 0.5) / 256.0, bytes=True)[:, :3].astype(np.uint8)
        cases = [(special_input(rng, lo, hi), (lo, hi)) for lo, hi in RANGES]
        cases.append((rng.standard_normal((5, 7)).astype(np.float32), (-2.5, 1.75)))
        cases.append((rng.standard_normal((5, 7)).astype(np.float32), None))                 # range from the data
        cases.append((np.full((5, 7), 0.375, np.float32), None))                             # constant frame, span 0
        for d, vrange in cases:
            vmin, vmax = (np.min(d), np.max(d)) if vrange is None else vrange
            with np.errstate(invalid="ignore", divide="ignore"):
                x = np.clip((d - vmin) / (vmax - vmin), 0.0, 1.0)
            assert x.dtype == np.float32
            out[f"input_{i}"] = d
            out[f"range_{i}"] = np.array([np.nan, np.nan] if vrange is None else vrange, np.float64)
            out[f"cmap_{i}"] = np.array(name)
            out[f"frame_{i}"] = cmap(x, bytes=True)[..., :3].astype(np.uint8)
            i += 1
    out["n_cases"] = np.array(i)
    path = os.path.join(HERE, "reference_frames.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {i} cases, {os.path.getsize(path)} bytes, matplotlib {matplotlib.__version__}")


if __name__ == "__main__":
    main()
