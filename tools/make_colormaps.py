"""Writes ``fluidgym_amd/envs/colormaps.json``: the 256-entry RGB tables of the colour maps that ship with the package, sampled from
matplotlib (``fluidgym_amd.envs.frames.sample_colormap``: the bytes the map gives to the centres of 256 equal bins of [0, 1], which for
these 256-entry maps is their table).  Run it again when a map is added to ``SHIPPED_COLORMAPS``; ``tests/test_frames_host.py`` holds
the file against the installed matplotlib.

    python tools/make_colormaps.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main() -> None:
    import matplotlib

    from fluidgym_amd.envs.frames import SHIPPED_COLORMAPS, sample_colormap

    tables = {name: sample_colormap(matplotlib.colormaps[name]) for name in SHIPPED_COLORMAPS}
    path = os.path.join(ROOT, "fluidgym_amd", "envs", "colormaps.json")
    with open(path, "w") as f:       # text, one line per map: the table's 768 bytes as hexadecimal digits
        f.write("{\n" + ",\n".join(f' "{name}": "{t.tobytes().hex()}"' for name, t in tables.items()) + "\n}\n")
    print(f"{path}: {', '.join(tables)} ({os.path.getsize(path)} bytes, matplotlib {matplotlib.__version__})")


if __name__ == "__main__":
    main()
