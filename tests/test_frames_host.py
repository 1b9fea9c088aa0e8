"""RGB frames, what holds without a GPU: the NumPy checker against matplotlib's own bytes, the colour tables,
the library's export and argument checks, the recording's files, the cylinder mask."""
import ctypes
import os
import warnings

import numpy as np
import pytest
import torch

import fluidgym_amd
from fluidgym_amd import _lib as L
from fluidgym_amd.envs import frames as F

from tests import frames_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_frames.npz")


def golden_cases():
    """(input, (lo32, span32), table, frame) of every case of the golden file."""
    g = np.load(GOLDEN)
    for i in range(int(g["n_cases"])):
        d, r = g[f"input_{i}"], g[f"range_{i}"]
        lo_span = R.auto_range(d) if np.isnan(r[0]) else R.fixed_range(float(r[0]), float(r[1]))
        yield i, d, r, lo_span, g["table_" + str(g[f"cmap_{i}"])], g[f"frame_{i}"]


def test_reference_restatement_equals_matplotlib_bytes():
    n = 0
    for i, d, r, lo_span, table, frame in golden_cases():
        assert d.dtype == np.float32 and frame.dtype == np.uint8 and frame.shape == d.shape + (3,)
        got = R.lookup(R.normalise(d, *lo_span), table)
        assert np.array_equal(got, frame), f"case {i}: {int((got != frame).any(-1).sum())} pixels differ"
        # the same through the kernel's restatement (a one-env, one-channel 2-D field, no orientation)
        assert np.array_equal(R.colorize(d[None, None, None], 0, -1, 0, False, False, False, table, [lo_span])[0], frame)
        n += 1
    assert n == 12
    # what the inputs were built to hold: a span of zero blacks the constant frame out, NaN is black, the infinities clip
    cases = {i: (d, frame) for i, d, _, _, _, frame in golden_cases()}
    assert not cases[5][1].any() and not cases[11][1].any()
    d, frame = cases[0]
    table = np.load(GOLDEN)["table_viridis"]
    flat, px = d.reshape(-1), frame.reshape(-1, 3)
    assert np.isnan(flat[257]) and not px[257].any()
    assert np.array_equal(px[258], table[255]) and np.array_equal(px[259], table[0]) and np.array_equal(px[260], table[0])
    assert np.array_equal(px[:257], table[np.minimum(np.arange(257), 255)])          # every tie k / 256 lands in bin k


def test_shipped_tables_equal_matplotlib():
    matplotlib = pytest.importorskip("matplotlib")
    for name in F.SHIPPED_COLORMAPS:
        table = F.resolve_colormap(name)
        assert table.dtype == np.uint8 and table.shape == (256, 3)
        assert np.array_equal(table, F.sample_colormap(matplotlib.colormaps[name])), name
        x = np.linspace(0, 1, 1001, dtype=np.float32)
        assert np.array_equal(R.lookup(x, table), matplotlib.colormaps[name](x, bytes=True)[:, :3])
    g = np.load(GOLDEN)
    assert np.array_equal(F.resolve_colormap("viridis"), g["table_viridis"]) and np.array_equal(F.resolve_colormap("rainbow"), g["table_rainbow"])


def test_resolve_colormap_tables_errors_and_icefire_fallback():
    table = np.arange(768, dtype=np.uint8).reshape(256, 3)
    assert F.resolve_colormap(table) is not None and np.array_equal(F.resolve_colormap(table), table)
    assert np.array_equal(F.resolve_colormap(torch.from_numpy(table)), table)
    with pytest.raises(ValueError, match="uint8 \\[256, 3\\]"):
        F.resolve_colormap(table.astype(np.float32))
    with pytest.raises(ValueError, match="uint8 \\[256, 3\\]"):
        F.resolve_colormap(table[:255])
    with pytest.raises(ValueError, match="seaborn or matplotlib"):
        F.resolve_colormap("no_such_colour_map")
    try:
        import seaborn as sns
    except ImportError:
        sns = None
    F._icefire_warned = False
    F._resolved.pop("icefire", None)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        first, second = F.resolve_colormap("icefire"), F.resolve_colormap("icefire")
    if sns is None:      # the fallback: coolwarm, said once
        assert np.array_equal(first, F.resolve_colormap("coolwarm")) and np.array_equal(second, first)
        assert [str(w.message) for w in caught if "icefire" in str(w.message)] == [
            "colour map 'icefire' is seaborn's and seaborn is not installed: using 'coolwarm' instead"]
    else:
        assert np.array_equal(first, F.sample_colormap(sns.color_palette("icefire", as_cmap=True))) and not caught


def _spec_frames(specs, field, lo_span, table):
    """The frames the kernel's restatement draws for key -> FrameSpec on a one-env field ``[C, nz, ny, nx]``."""
    return {key: R.colorize(field[None], s.channel, s.axis, s.index, s.transpose, s.flip_rows, s.flip_cols, table, [lo_span])[0]
            for key, s in specs.items()}


def test_family_specs_are_the_reference_recipes_on_unequal_extents():
    """The folded specs of every family against the recipes written with the reference's own index expressions, on fields whose
    z, y and x extents all differ (so an index taken from the wrong axis, or a mid plane where the lines say plane 1, shows)."""
    rng = np.random.default_rng(11)
    table = F.resolve_colormap("viridis")
    nz, ny, nx = 6, 5, 9
    same = lambda got, want: list(got) == list(want) and all(got[k].shape == want[k].shape and np.array_equal(got[k], want[k]) for k in want)
    T = rng.uniform(-0.2, 2.0, (1, nz, ny, nx)).astype(np.float32)
    assert same(_spec_frames(F.rbc_frame_specs(3, (nz, ny, nx)), T, R.fixed_range(0.0, 1.75), table), R.rbc_frames(T[0], 0.0, 1.75, table))
    assert same(_spec_frames(F.rbc_frame_specs(2, (ny, nx)), T[:, :1], R.fixed_range(0.0, 1.75), table), R.rbc_frames(T[0, 0], 0.0, 1.75, table))
    w = rng.uniform(-12, 12, (3, nz, ny, nx)).astype(np.float32)
    assert same(_spec_frames(F.vortex_frame_specs(3, (nz, ny, nx), False), w, R.fixed_range(-10, 10), table), R.cylinder_frames(w, table, None))
    assert same(_spec_frames(F.vortex_frame_specs(3, (nz, ny, nx), True), w, R.fixed_range(-12.5, 12.5), table),
                R.airfoil_frames(w, table, (-12.5, 12.5)))
    assert same(_spec_frames(F.vortex_frame_specs(2, (ny, nx), True), w[:1, :1], R.fixed_range(-10, 10), table),
                R.airfoil_frames(w[:1, 0], table, (-10, 10)))
    # the literal planes: z plane 1, y index nz // 2 = 3, x index int(ny * 0.8) = 4 of the x-flipped field
    cyl = F.vortex_frame_specs(3, (nz, ny, nx), False)
    assert (cyl["x-y-vorticity"].index, cyl["x-z-vorticity"].index, cyl["y-z-vorticity"].index) == (1, 3, nx - 1 - 4)
    u = rng.uniform(-0.6, 0.6, (3, nz, ny, nx)).astype(np.float32)
    specs = F.tcf_frame_specs((nz, ny, nx), wall_row=1)
    got = _spec_frames({k: v for k, v in specs.items() if k.endswith("velocity")}, u, R.fixed_range(0.0, 0.9), table)
    got.update(_spec_frames({k: v for k, v in specs.items() if k.endswith("vorticity")}, w, R.auto_range(w, symmetric=True), table))
    assert same(got, R.tcf_frames(u, w, 1, 0.9, table, table))
    assert (specs["x-y-vorticity"].index, specs["y-z-vorticity"].index, specs["x-y-velocity"].index, specs["y-z-velocity"].index) == (
        1, nx - 1 - ny // 2, nz // 2, nx - 1 - nx // 2)


def test_frame_spec_mirrors_the_c_struct():
    spec = F.FrameSpec(channel=-1, axis=2, index=3, transpose=True, flip_rows=False, flip_cols=True)
    c = spec.c_struct()
    assert [name for name, _ in L.FgFrameSpec._fields_] == ["channel", "axis", "index", "transpose", "flip_rows", "flip_cols"]
    assert (c.channel, c.axis, c.index, c.transpose, c.flip_rows, c.flip_cols) == (-1, 2, 3, 1, 0, 1)
    assert ctypes.sizeof(L.FgFrameSpec) == 24
    assert spec.frame_shape(4, 5, 6) == (5, 4)                      # rows z, cols y, transposed
    assert F.FrameSpec(axis=1).frame_shape(4, 5, 6) == (4, 6) and F.FrameSpec().frame_shape(1, 5, 6) == (5, 6)


def test_library_exports_frame_colorize_in_the_fp32_build_only():
    assert hasattr(L.load(), "fg_frame_colorize") and "fg_frame_colorize" in L.SIGNATURES
    assert "fg_frame_colorize" not in L.SIGNATURES_F64 and not hasattr(L.load_f64(), "fg_frame_colorize")


def test_argument_checks_answer_before_any_launch():
    """Every check of fg_frame_colorize answers FG_ERR_INVALID_ARG with a message, on a machine without a GPU: the pointers below are
    host arrays the library must never get to read (only envs, which is a host array by contract)."""
    lib = L.load()
    B, C, nz, ny, nx = 3, 2, 4, 5, 6
    field = np.zeros((B, C, nz, ny, nx), np.float32)
    table, rng, out = np.zeros((256, 3), np.uint8), np.zeros((2, 2), np.float32), np.zeros((2, 5, 6, 3), np.uint8)
    envs = np.array([2, 0], np.int32)

    def call(spec=(0, 0, 0, 0, 0, 0), envs_=envs, n=2, shape=(B, C, nz, ny, nx), null=()):
        s = L.FgFrameSpec(*spec)
        ptr = lambda name, a: None if name in null else ctypes.c_void_p(a.ctypes.data)
        rc = lib.fg_frame_colorize(ptr("field", field), *shape, None if "spec" in null else ctypes.byref(s), ptr("table", table), None,
                                   ptr("range", rng), None if "envs" in null else envs_.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), n,
                                   ptr("out", out), None)
        return rc, lib.fg_last_error().decode()

    for name in ("field", "spec", "table", "range", "envs", "out"):
        rc, msg = call(null=(name,))
        assert rc == L.FG_ERR_INVALID_ARG and "null" in msg, name
    cases = [
        (dict(n=0), "n must be"),
        (dict(shape=(B, C, nz, 0, nx)), "extent"),
        (dict(envs_=np.array([0, 3], np.int32)), "envs[1] = 3"),
        (dict(envs_=np.array([-1, 0], np.int32)), "envs[0] = -1"),
        (dict(spec=(2, 0, 0, 0, 0, 0)), "channel 2"),
        (dict(spec=(-2, 0, 0, 0, 0, 0)), "channel -2"),
        (dict(spec=(0, 3, 0, 0, 0, 0)), "axis"),
        (dict(spec=(0, -2, 0, 0, 0, 0)), "axis"),
        (dict(spec=(0, -1, 0, 0, 0, 0)), "nz == 1"),
        (dict(spec=(0, -1, 1, 0, 0, 0), shape=(B, C, 1, ny, nx)), "index 1"),
        (dict(spec=(0, 0, 4, 0, 0, 0)), "index 4"),
        (dict(spec=(0, 1, 5, 0, 0, 0)), "index 5"),
        (dict(spec=(0, 2, 6, 0, 0, 0)), "index 6"),
        (dict(spec=(0, 2, -1, 0, 0, 0)), "index -1"),
    ]
    for kw, needle in cases:
        rc, msg = call(**kw)
        assert rc == L.FG_ERR_INVALID_ARG and needle in msg and msg.startswith("fg_frame_colorize"), (kw, msg)
    assert not out.any()
    # the Python door refuses a view that is not on the GPU: there is no CPU path
    with pytest.raises(L.NativeLibraryError, match="no CPU path"):
        F.colorize(torch.zeros(1, 1, 4, 4), F.FrameSpec(), "viridis", (0, 1))


def _recording():
    rng = np.random.default_rng(3)
    frames = {"vorticity": rng.integers(0, 256, (3, 2, 5, 7, 3), dtype=np.uint8), "x-y-velocity": rng.integers(0, 256, (3, 2, 4, 4, 3), dtype=np.uint8)}
    return F.FrameRecording(frames, envs=(1, 0), steps=(0, 2, 4), fps=24)


def test_recording_png_and_gif_round_trip(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    rec = _recording()
    assert len(rec) == 3 and rec.envs == [1, 0] and rec.steps == [0, 2, 4]
    written = rec.save_png(tmp_path / "png", env=0, t=1)
    assert sorted(p.name for p in written.values()) == ["vorticity_env0_000002.png", "x-y-velocity_env0_000002.png"]
    for key, path in written.items():
        assert np.array_equal(np.asarray(Image.open(path).convert("RGB")), rec.frames[key][1, 1])      # env 0 is column 1
    one = rec.save_gif("episode.gif", tmp_path / "gif", env=1)
    assert sorted(p.name for p in one.values()) == ["vorticity_episode.gif", "x-y-velocity_episode.gif"]       # the reference's naming
    both = rec.save_gif("run", tmp_path / "gif")
    assert sorted(p.name for p in both.values()) == ["vorticity_env0_run.gif", "vorticity_env1_run.gif", "x-y-velocity_env0_run.gif",
                                                     "x-y-velocity_env1_run.gif"]
    gif = Image.open(one[("vorticity", 1)])
    assert gif.n_frames == 3 and gif.size == (7, 5) and gif.info["duration"] in (40, 41, 42)      # 1000 / 24 ms, in GIF's 10 ms ticks
    # a frame of few colours survives the palette exactly
    flat = np.zeros((2, 1, 4, 6, 3), np.uint8)
    flat[0, 0, :, :3] = (255, 0, 0)
    flat[1, 0, 2:] = (0, 0, 255)
    path = F.FrameRecording({"k": flat}, envs=(0,), steps=(0, 1)).save_gif("flat", tmp_path)[("k", 0)]
    gif = Image.open(path)
    for t in range(2):
        gif.seek(t)
        assert np.array_equal(np.asarray(gif.convert("RGB")), flat[t, 0])
    with pytest.raises(ValueError, match="not recorded"):
        rec.save_png(tmp_path, env=5)
    with pytest.raises(ValueError, match="uint8"):
        F.FrameRecording({"k": flat.astype(np.float32)}, envs=(0,), steps=(0, 1))


@pytest.mark.parametrize("env_id, ndims", [("CylinderJet2D-easy-v0", 2), ("CylinderJet3D-easy-v0", 3)])
def test_cylinder_mask_is_the_reference_formula(env_id, ndims):
    env = fluidgym_amd.make(env_id, resolution=8, cuda_device=torch.device("cpu"))
    mask = env._get_cylinder_mask()
    shape = env.render_shape
    assert shape == (171, 32, 32)
    want = R.cylinder_mask(shape, ndims)
    assert mask.dtype == bool and mask.shape == ((32, 32, 171) if ndims == 3 else (32, 171)) and np.array_equal(mask, want)
    disc = mask[0] if ndims == 3 else mask
    # a disc of radius 0.5 / 4.1 * 31 = 3.78 pixels about pixel (15, 15)
    assert disc[15, 15] and disc[15, 18] and disc[12, 15] and not disc[15, 19] and not disc[11, 15] and int(disc.sum()) == 45
    assert not disc[:, 0].any() and not disc[0].any()          # the 3-D slices mask[:, 0, :] and mask[:, :, 0] hold no solid pixel
