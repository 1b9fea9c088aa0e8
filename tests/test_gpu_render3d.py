"""3-D frames on the GPU: ``fg_render_isosurface`` / ``fg_render_volume`` and the envs' ``render_frames_3d``
against the NumPy restatement ``tests/render3d_ref.py``.  The contract is equality, bytes and depth: there is no tolerance in this
file."""
import numpy as np
import pytest
import torch

import fluidgym_amd
from fluidgym_amd.envs import frames as F
from fluidgym_amd.envs import render3d as R3
from tests import render3d_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
TABLE = F.resolve_colormap("rainbow")
SHAPE = (5, 6, 7)                  # nz, ny, nx of the small volume [3, 2, 5, 6, 7]
SIZE = (9, 13)                     # no multiple of the 16 x 16 tile


def small_volume(seed=1):
    """``[3, 2, 5, 6, 7]``: smooth blobs plus noise, so that a level near 1 has a surface inside the box in every env."""
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in SHAPE), indexing="ij")
    vol = np.empty((3, 2) + SHAPE, np.float32)
    for b in range(3):
        for c in range(2):
            cx, cy, cz = rng.uniform(1.5, 4.5), rng.uniform(1.5, 3.5), rng.uniform(1.0, 3.0)
            vol[b, c] = 2.2 * np.exp(-((x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2) / 5.0) - 0.4 + 0.1 * rng.standard_normal(SHAPE)
    return vol


def cameras():
    """name -> (camera, size): both projections of an oblique orbit, parallel rays along each axis exactly (spaced so that rays run
    along faces and edges of the box), an oblique hand-made view, and an eye inside the box."""
    H, W = SIZE
    out = {p: R3.orbit_camera(SHAPE, (7.0, 6.0, 5.0), 20, 50, size=SIZE, projection=p, zoom=1.6) for p in ("persp", "ortho")}
    z3 = (0, 0, 0)
    out["along_x"] = R3.camera_from_vectors((-1.5, -0.75, -0.75), (0, 0.5, 0), (0, 0, 0.5), (1, 0, 0), z3, z3)      # j = 1: y = 0, i = 1: z = 0
    out["against_y"] = R3.camera_from_vectors((-0.75, 7.0, -0.25), (0.625, 0, 0), (0, 0, 0.5), (0, -1, 0), z3, z3)
    out["along_z"] = R3.camera_from_vectors((-0.25, 5.25, -2.0), (0.5, 0, 0), (0, -0.625, 0), (0, 0, 2), z3, z3)       # j = 0 ... x = 0; a longer d
    out["inside"] = R3.camera_from_vectors((3.0, 2.5, 2.0), z3, z3, (1.0, -0.45, -0.6), (0, 0.07, 0.01), (0, -0.01, 0.13))
    return {k: (c, SIZE) for k, c in out.items()}


CAMERAS = cameras()


def step_of(cam):
    return 0.5 / float(np.linalg.norm(R3.camera_array(cam)[3].astype(np.float64)))


def check_iso(vol, channel, level, cvol, cchannel, color_range, cam, size, clip=None, solid=None, envs=None, step=None):
    """Kernel against restatement, frames and depth, with equality.  Returns (frames, depth) of the kernel on the host."""
    H, W = size
    step = np.float32(step_of(cam) if step is None else step)
    listed = list(range(vol.shape[0])) if envs is None else list(envs)
    got, depth = R3.raycast_isosurface(torch.from_numpy(vol).to(DEV), channel, level, torch.from_numpy(cvol).to(DEV), cchannel, color_range,
                                       torch.from_numpy(TABLE).to(DEV), cam, clip=clip, solid=solid, envs=envs, return_depth=True,
                                       size=size, step=float(step))
    assert got.dtype == torch.uint8 and tuple(got.shape) == (len(listed), H, W, 3) and got.is_cuda
    assert depth.dtype == torch.float32 and tuple(depth.shape) == (len(listed), H, W)
    levels = np.broadcast_to(np.asarray(level, np.float32).reshape(-1), (vol.shape[0],))[listed]
    if isinstance(color_range, str):
        ranges = [R.auto_range(R.scalar_field(cvol[e], cchannel)) for e in listed]
    else:
        ranges = [R.fixed_range(*color_range)] * len(listed)
    want, want_depth = R.isosurface(vol, channel, levels, cvol, cchannel, ranges, TABLE, R3.camera_array(cam), H, W, step, clip=clip,
                                    solid=solid, envs=listed)
    got, depth = got.cpu().numpy(), depth.cpu().numpy()
    bad = depth.view(np.uint32) != want_depth.view(np.uint32)
    assert not bad.any(), f"{int(bad.sum())} of {bad.size} depths differ, first at {np.argwhere(bad)[0]}: {depth[bad][0]!r} != {want_depth[bad][0]!r}"
    diff = (got != want).any(-1)
    assert not diff.any(), f"{int(diff.sum())} of {diff.size} pixels differ, first at {np.argwhere(diff)[0]}"
    return got, depth


def check_volume(vol, channel, value_range, opacity, cam, size, envs=None, background=(255, 255, 255)):
    H, W = size
    step = np.float32(step_of(cam))
    listed = list(range(vol.shape[0])) if envs is None else list(envs)
    got = R3.raycast_volume(torch.from_numpy(vol).to(DEV), channel, value_range, torch.from_numpy(TABLE).to(DEV), opacity, cam,
                            background=background, envs=envs, size=size, step=float(step))
    assert got.dtype == torch.uint8 and tuple(got.shape) == (len(listed), H, W, 3) and got.is_cuda
    want = R.volume(vol, channel, [R.fixed_range(*value_range)] * len(listed), TABLE, opacity, R3.camera_array(cam), H, W, step,
                    background=background, envs=listed)
    got = got.cpu().numpy()
    diff = (got != want).any(-1)
    assert not diff.any(), f"{int(diff.sum())} of {diff.size} pixels differ, first at {np.argwhere(diff)[0]}"
    return got


@pytest.mark.parametrize("name", list(CAMERAS))
def test_small_volume_every_camera_one_channel_and_the_norm(name):
    cam, size = CAMERAS[name]
    vol = small_volume()
    hits = 0
    for channel, cchannel in ((0, 1), (-1, -1), (1, 0)):
        _, depth = check_iso(vol, channel, 0.9, vol, cchannel, (-0.5, 2.5), cam, size)
        hits += int(np.isfinite(depth).sum())
    assert hits > 20, "no camera of this file may look past the surface"


def test_env_lists_levels_per_env_and_a_level_out_of_reach():
    cam, size = CAMERAS["persp"]
    vol = small_volume(2)
    check_iso(vol, 0, 0.9, vol, 1, "auto", cam, size, envs=[2, 0, 2, 1, 1])                 # out of order, repeats, a range per env
    a, da = check_iso(vol, -1, [0.6, 0.9, 1.2], vol, 0, (-0.5, 2.5), cam, size)               # one level per env
    b, db = check_iso(vol, -1, [1.2, 0.9, 0.6], vol, 0, (-0.5, 2.5), cam, size, envs=[2, 1, 0])
    assert np.array_equal(a[1], b[1]) and not np.array_equal(da[0], db[2])
    got, depth = check_iso(vol, 0, 50.0, vol, 0, (-0.5, 2.5), cam, size)                      # a level no sample reaches
    assert (got == 255).all() and np.isposinf(depth).all()


def test_more_listed_envs_than_one_launch_takes():
    rng = np.random.default_rng(5)
    vol = rng.uniform(0, 2, (5, 1, 3, 3, 3)).astype(np.float32)
    envs = [int(e) for e in rng.integers(0, 5, 131)]                                          # 64 + 64 + 3
    cam = R3.orbit_camera((3, 3, 3), (1, 1, 1), 20, 50, size=(5, 6), zoom=1.5)
    levels = [0.7, 0.9, 1.0, 1.1, 1.3]
    check_iso(vol, 0, levels, vol, 0, (0, 2), cam, (5, 6), envs=envs)
    check_volume(vol, 0, (0, 2), R3.log_opacity_table(0.3), cam, (5, 6), envs=envs)


def test_nan_and_infinities_sown_in():
    vol = small_volume(3)
    flat = vol.reshape(-1)
    rng = np.random.default_rng(4)
    flat[rng.choice(flat.size, 24, replace=False)] = np.tile(np.array([np.nan, np.inf, -np.inf], np.float32), 8)
    for name in ("persp", "along_x", "inside"):
        cam, size = CAMERAS[name]
        check_iso(vol, 0, 0.9, vol, 1, (-0.5, 2.5), cam, size)
        check_iso(vol, -1, 0.9, vol, -1, "auto", cam, size)                                   # a NaN range: black where the surface is hit
        check_volume(vol, 0, (-0.5, 2.5), R3.log_opacity_table(0.3), cam, size)


def test_clip_boxes():
    vol = small_volume()
    for name in ("persp", "against_y"):
        cam, size = CAMERAS[name]
        full, dfull = check_iso(vol, 0, 0.9, vol, 1, (-0.5, 2.5), cam, size)
        whole, dwhole = check_iso(vol, 0, 0.9, vol, 1, (-0.5, 2.5), cam, size, clip=((0, 0, 0), (6, 5, 4)))      # the whole box
        assert np.array_equal(full, whole) and np.array_equal(dfull, dwhole)
        check_iso(vol, 0, 0.9, vol, 1, (-0.5, 2.5), cam, size, clip=((3, 2, 2), (4, 3, 3)))                       # one cell
        cut, dcut = check_iso(vol, 0, 0.9, vol, 1, (-0.5, 2.5), cam, size, clip=((0, 0, 0), (6, 2.5, 4)))         # through the surface
        assert not np.array_equal(dcut, dfull)
    # seen from above, the cut-open surface has no cap: rays that enter the clip box inside the iso region pass on to its far side
    cam, size = CAMERAS["against_y"]
    _, dcut = check_iso(vol, 0, 0.9, vol, 1, (-0.5, 2.5), cam, size, clip=((0, 0, 0), (6, 2.5, 4)))
    assert (dcut[np.isfinite(dcut)] >= 7.0 - 2.5).all()                                         # (the camera sits at y = 7, d = -y)


def test_solid_body_in_front_behind_and_through_the_surface():
    vol = small_volume()
    cam, size = CAMERAS["along_x"]
    plain, dplain = check_iso(vol, 0, 0.9, vol, 1, (-0.5, 2.5), cam, size)
    for name, region in (("front", (slice(None), slice(None), slice(0, 1))), ("behind", (slice(None), slice(None), slice(6, 7))),
                         ("through", (slice(1, 4), slice(2, 4), slice(2, 5)))):
        solid = np.zeros(SHAPE, np.uint8)
        solid[region] = 1
        got, depth = check_iso(vol, 0, 0.9, vol, 1, (-0.5, 2.5), cam, size, solid=solid)
        for other in ("persp", "inside"):
            check_iso(vol, -1, 0.9, vol, 0, (-0.5, 2.5), *CAMERAS[other], solid=solid, clip=((1, 1, 1), (5, 4, 3)))
        hit = np.isfinite(depth)
        if name == "front":               # the slab x < 0.5 hides everything behind it
            inside = np.isfinite(depth[0])
            assert inside.any() and np.all(depth[0][inside] < 1.5 + 0.6)
        if name == "behind":              # the surface stays where it was; rays that missed it end on the slab
            seen = np.isfinite(dplain)
            assert np.array_equal(depth[seen], dplain[seen]) and hit.sum() > seen.sum()
        if name == "through":
            assert not np.array_equal(depth, dplain) and (np.minimum(depth, dplain) == depth).all()


@pytest.mark.parametrize("size", [(1, 1), (16, 16), (17, 33)], ids=lambda s: "x".join(map(str, s)))
def test_image_sizes(size):
    vol = small_volume()
    for projection in ("persp", "ortho"):
        cam = R3.orbit_camera(SHAPE, (7.0, 6.0, 5.0), 20, 50, size=size, projection=projection, zoom=1.6)
        check_iso(vol, 0, 0.9, vol, 1, (-0.5, 2.5), cam, size)
        check_volume(vol, -1, (0.0, 2.5), R3.log_opacity_table(0.3), cam, size, envs=[1])


@pytest.mark.parametrize("name", list(CAMERAS))
def test_volume_mode_log_zero_and_full_opacity(name):
    """The log table, a table of zeros (the background) and a table of ones (the first sample's colour; the march stops at once):
    early termination must not change a byte against the restatement."""
    cam, size = CAMERAS[name]
    vol = small_volume()
    background = (12, 34, 56)
    for channel in (0, -1):
        got = check_volume(vol, channel, (-0.5, 2.5), R3.log_opacity_table(0.3), cam, size, background=background)
        assert len(np.unique(got.reshape(-1, 3), axis=0)) > 4
        dense = check_volume(vol, channel, (-0.5, 2.5), R3.log_opacity_table(1.0), cam, size, background=background)      # reaches the cut-off
        assert not np.array_equal(dense, got)
    zero = check_volume(vol, 0, (-0.5, 2.5), np.zeros(256, np.float32), cam, size, envs=[2, 0], background=background)
    assert (zero == np.array(background, np.uint8)).all()
    check_volume(vol, 0, (-0.5, 2.5), np.ones(256, np.float32), cam, size, background=background)


def test_python_doors_refuse_what_the_library_would():
    view = torch.zeros(2, 2, 3, 4, 5, device=DEV)
    cam = R3.orbit_camera((3, 4, 5), (1, 1, 1), 15, 60, size=(4, 4))
    with pytest.raises(ValueError, match="envs must lie"):
        R3.raycast_isosurface(view, 0, 0.5, view, 0, (0, 1), "rainbow", cam, envs=[2])
    with pytest.raises(ValueError, match="level must be"):
        R3.raycast_isosurface(view, 0, [0.5, 0.6, 0.7], view, 0, (0, 1), "rainbow", cam)
    with pytest.raises(ValueError, match="solid mask"):
        R3.raycast_isosurface(view, 0, 0.5, view, 0, (0, 1), "rainbow", cam, solid=np.zeros((3, 4, 4), np.uint8))
    with pytest.raises(fluidgym_amd._lib.NativeLibraryError, match="channel 2"):
        R3.raycast_volume(view, 2, (0, 1), "rainbow", R3.log_opacity_table(), cam)
    with pytest.raises(fluidgym_amd._lib.NativeLibraryError, match="clip box is empty"):
        R3.raycast_isosurface(view, 0, 0.5, view, 0, (0, 1), "rainbow", cam, clip=((2, 0, 0), (1, 3, 2)))
    with pytest.raises(ValueError, match="opacity table"):
        R3.raycast_volume(view, 0, (0, 1), "rainbow", np.zeros(255, np.float32), cam)


# ------------------------------------------------------------------------------------------------ env level
# the small configurations of tests/test_gpu_frames.py; the cylinder at resolution 12 after 40 steps of development, the smallest at which
# the family's own clip box (15 <= y < ny - 15 of a render grid of ny = 4 resolution rows) holds more than the wake's centre line and the
# vorticity inside it passes the family's level: at resolution 8 the clip box is the rows 15 and 16 and no sample in it reaches 1.5
CYL3 = dict(resolution=12, n_jets=4, initial_domain_steps=40, randomize_initial_state=False, step_length=0.03, dt=0.01, episode_length=4)
AIRFOIL3 = dict(initial_domain_steps=4, randomize_initial_state=False, episode_length=2, resolution_div=4, res_z=8, n_agents=4)
ENVS = {
    "RBC3D-easy-v0": dict(num_envs=2, n_heaters=2, resolution=4, use_marl=False, step_length=0.1, load_initial_domain=False,
                          load_domain_statistics=False),
    "CylinderJet3D-easy-v0": dict(num_envs=2, **CYL3),
    "TCFSmall3D-both-easy-v0": dict(num_envs=2, resolution_x_z=16, resolution_y=16, step_length=0.6, use_marl=False,
                                    randomize_initial_state=False),
}
KEYS = {"RBC3D": "3d_temperature", "CylinderJet3D": "3d_vorticity", "TCF": "3d_q_criterion"}
SMALL = (24, 32)


class drawn_specs:
    """Collects the specs ``render_frames_3d`` actually draws from while the block runs, their tensors cloned: the checker is applied
    to THESE views, not to a second evaluation of the accessors (the 3-D multi-block resampler sums with atomics, so two calls of
    ``get_vorticity()`` may differ in the last bit; equality is asked of the ray marcher, not of that sum's order)."""

    def __init__(self, env):
        self.env, self.calls = env, []

    def __enter__(self):
        inner = self.env._frame_specs_3d

        def spy():
            specs = inner()
            self.calls.append({key: {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in s.items()} for key, s in specs.items()})
            return specs

        self.env._frame_specs_3d = spy
        return self

    def __exit__(self, *exc):
        del self.env._frame_specs_3d


def reference_frame_3d(spec, envs, size, projection="persp"):
    """The restatement applied to the views of a spec, with the spec's own level, colour field, range, map, clip, solid and view."""
    host = lambda t: t.detach().to(torch.float32).cpu().numpy()
    vol = host(spec["view"])
    cam = R3.orbit_camera(vol.shape[2:], spec["extent"], spec["elev"], spec["azim"], size=size, projection=projection)
    step, table = np.float32(R3.default_step(cam)), F.resolve_colormap(spec["cmap"])
    if spec["mode"] == "volume":
        return R.volume(vol, spec["channel"], [R.fixed_range(*spec["range"])] * len(envs), table, spec["opacity"], R3.camera_array(cam),
                        *size, step, envs=envs)
    cvol = host(spec["color_view"])
    if isinstance(spec["color_range"], str):
        ranges = [R.auto_range(R.scalar_field(cvol[e], spec["color_channel"])) for e in envs]
    else:
        ranges = [R.fixed_range(*spec["color_range"])] * len(envs)
    solid = None if spec["solid"] is None else spec["solid"].cpu().numpy()
    levels = np.broadcast_to(np.asarray(spec["level"], np.float32).reshape(-1), (vol.shape[0],))[list(envs)]
    return R.isosurface(vol, spec["channel"], levels, cvol, spec["color_channel"], ranges, table, R3.camera_array(cam), *size, step,
                        clip=spec["clip"], solid=solid, body=R3.BODY_COLOR, envs=envs)[0]


def grey(frame):
    """Pixels of the shaded body (the body colour is a grey, the background white, the ``rainbow`` table holds no grey)."""
    return (frame[..., 0] == frame[..., 1]) & (frame[..., 1] == frame[..., 2]) & (frame[..., 0] < 255)


def assert_same_or_neighbouring_bins(a, b, table, what):
    """Two frames of one state drawn from two evaluations of a view that may differ in the last bits (the 3-D multi-block resampler
    sums with atomics): a pixel changes only where ``x 256`` lies within the view's rounding of an integer, and then to the
    neighbouring bin.  With a view good to ``k`` ulp that is a share of about ``256 k 2^-23`` of the pixels, 5e-4 for the 16 summands
    of a resampled cell; the bound here is 1 % of the pixels, none by more than one bin of the table."""
    diff = (a != b).any(-1)
    assert diff.sum() <= 0.01 * diff.size, f"{what}: {int(diff.sum())} of {diff.size} pixels differ"
    where = {}
    for k, c in enumerate(table):
        where.setdefault(tuple(int(v) for v in c), []).append(k)
    for pa, pb in zip(a[diff], b[diff]):
        ka, kb = where[tuple(int(v) for v in pa)], where[tuple(int(v) for v in pb)]
        assert min(abs(i - j) for i in ka for j in kb) <= 1, f"{what}: a pixel moved from bin {ka} to bin {kb}"


@pytest.mark.filterwarnings("ignore:colour map 'icefire'")
@pytest.mark.parametrize("env_id", list(ENVS))
def test_env_frames_3d(env_id, tmp_path):
    env = fluidgym_amd.make(env_id, **ENVS[env_id])
    key = next(v for k, v in KEYS.items() if env_id.startswith(k))
    with pytest.raises(RuntimeError, match="reset"):
        env.render_frames_3d()
    env.reset(seed=3)
    zero = torch.zeros_like(env.sample_action())
    env.step(zero)
    flat = {k: v.cpu().numpy() for k, v in env.render_frames().items()}                      # before the new path was ever used
    with drawn_specs(env) as seen:
        frames = env.render_frames_3d(size=SMALL)
    assert list(frames) == [key] and len(seen.calls) == 1
    got = frames[key]
    assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == (2,) + SMALL + (3,)
    got = got.cpu().numpy()
    want = reference_frame_3d(seen.calls[0][key], [0, 1], SMALL)
    diff = (got != want).any(-1)
    assert not diff.any(), f"{key}: {int(diff.sum())} of {diff.size} pixels differ"
    assert len(np.unique(got.reshape(-1, 3), axis=0)) > 2, "the picture is flat"
    if env_id.startswith("CylinderJet3D"):      # the family's level, clip and colour range meet a surface of the real wake, beside the body
        surface = ~grey(got) & ~(got == 255).all(-1)
        assert surface.any(axis=(1, 2)).all() and grey(got).any(axis=(1, 2)).all(), (surface.sum(), grey(got).sum())
    # render_frames() gives byte for byte what it gave before render_frames_3d ran, where its views are reproducible from call to call;
    # the 3-D multi-block resampler sums with atomics: there the frames may differ as two calls of render_frames() may anyway
    again = {k: v.cpu().numpy() for k, v in env.render_frames().items()}
    assert list(again) == list(flat)
    if torch.equal(env.get_vorticity(), env.get_vorticity()) or not env_id.startswith("CylinderJet3D"):
        assert all(np.array_equal(again[k], flat[k]) for k in flat)
    else:
        for k, (_, _, _, default_map, _) in env._frame_specs().items():
            assert_same_or_neighbouring_bins(again[k], flat[k], F.resolve_colormap(default_map), k)
    # envs listed, the other projection, another view
    with drawn_specs(env) as seen:
        other = env.render_frames_3d(envs=[1], size=SMALL, view=dict(azim=120), projection="ortho")[key].cpu().numpy()
    spec = dict(seen.calls[0][key], azim=120)
    assert np.array_equal(other, reference_frame_3d(spec, [1], SMALL, "ortho")) and other.shape == (1,) + SMALL + (3,)

    # identical envs give identical frames, envs in different states different ones
    if env_id.startswith("RBC"):
        block = env._domain.getBlock(0)
        block.passiveScalar[1].copy_(block.passiveScalar[0])
        same = env.render_frames_3d(size=SMALL)[key].cpu().numpy()
        assert np.array_equal(same[0], same[1])
        block.passiveScalar[1].mul_(0.5)
        moved = env.render_frames_3d(size=SMALL)[key].cpu().numpy()
        assert np.array_equal(moved[0], same[0]) and not np.array_equal(moved[0], moved[1])
    elif env_id.startswith("TCF"):
        block = env._domain.getBlock(0)
        block.velocity[1].copy_(block.velocity[0])
        same = env.render_frames_3d(size=SMALL)[key].cpu().numpy()
        assert np.array_equal(same[0], same[1])
        block.velocity[1].mul_(0.5)
        moved = env.render_frames_3d(size=SMALL)[key].cpu().numpy()
        assert np.array_equal(moved[0], same[0]) and not np.array_equal(moved[0], moved[1])
    else:
        # the same state in both envs of this batch (no randomisation, the same action); the multi-block resampler's atomics decide the
        # last bits of each env's view on their own, so equality is asked of one set of views drawn twice
        with drawn_specs(env) as seen:
            env.render_frames_3d(size=SMALL)
        spec = seen.calls[0][key]
        spec["view"][1].copy_(spec["view"][0]); spec["color_view"][1].copy_(spec["color_view"][0])
        env._frame_specs_3d = lambda: {key: spec}
        same = env.render_frames_3d(size=SMALL)[key].cpu().numpy()
        assert np.array_equal(same[0], same[1])
        del env._frame_specs_3d
        assert np.array_equal(same[0], same[1])
        # env 1 at half the speed: its vorticity halves and the family's level meets another surface
        env._domain.velocity[1].mul_(0.5)
        with drawn_specs(env) as seen:
            moved = env.render_frames_3d(size=SMALL)[key].cpu().numpy()
        assert np.array_equal(moved, reference_frame_3d(seen.calls[0][key], [0, 1], SMALL))
        assert not np.array_equal(moved[1], got[1]) and not np.array_equal(moved[0], moved[1])

    # a recording with render_3d=True over two steps: T = 3 samples under the 2-D and the 3-D keys, and save_gif writes them
    env.start_frame_recording(envs=(1, 0), render_3d=True, size=SMALL)
    env.step(zero)
    env.step(zero)
    rec = env.stop_frame_recording()
    assert len(rec) == 3 and sorted(rec.frames) == sorted(list(flat) + [key])
    assert rec.frames[key].shape == (3, 2) + SMALL + (3,) and all(rec.frames[k].shape[:2] == (3, 2) for k in flat)
    written = rec.save_gif("episode", output_path=tmp_path, env=0)
    assert (key, 0) in written and all(p.exists() and p.stat().st_size > 0 for p in written.values())
    env.start_frame_recording()                                                               # the default leaves the samples as they were
    assert sorted(env.stop_frame_recording().frames) == sorted(flat)
    env.close()


def test_airfoil_env_frames_3d():
    """``Airfoil3D`` at its smallest mesh (the configuration of ``tests/test_gpu_airfoil.py``); its render grid is 600 x 150 x 150 at
    every ``resolution_div``, so one env and one step: ``make`` and ``reset`` take 10 s on an MI355X, there as here, and what this test
    adds to them takes 1 s.  The wing sits inside the surface its own boundary layer makes at the family's
    level (the family clips no x), so the family's picture shows that sheath; the body itself is shown by the same spec with the
    surface clipped away to a corner cell of the box."""
    env = fluidgym_amd.make("Airfoil3D-easy-v0", num_envs=1, **AIRFOIL3)
    env.reset(seed=3)
    env.step(torch.zeros_like(env.sample_action()))
    key = "3d_vorticity"
    with drawn_specs(env) as seen:
        frames = env.render_frames_3d(size=SMALL)
    assert list(frames) == [key] and len(seen.calls) == 1
    got = frames[key]
    assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == (1,) + SMALL + (3,)
    got, spec = got.cpu().numpy(), seen.calls[0][key]
    nz, ny, nx = spec["view"].shape[2:]
    assert (nz, ny, nx) == tuple(reversed(env.render_shape)) and spec["clip"] == ((0, 15, 0), (nx - 1, ny - 16, nz - 1))
    assert spec["level"] == 2.0 and spec["extent"] == (env.L + 1.5, env.H, env.D) and (spec["elev"], spec["azim"]) == (10, 60)
    solid = spec["solid"]
    assert tuple(solid.shape) == (nz, ny, nx) and solid.any() and torch.equal(solid[0], solid[-1])
    assert np.array_equal(got, reference_frame_3d(spec, [0], SMALL))
    assert (~(got == 255).all(-1)).any(), "no ray meets the surface round the wing"
    bare = dict(spec, clip=((0, 0, 0), (1, 1, 1)))
    env._frame_specs_3d = lambda: {key: bare}
    body = env.render_frames_3d(size=SMALL)[key].cpu().numpy()
    del env._frame_specs_3d
    assert np.array_equal(body, reference_frame_3d(bare, [0], SMALL))
    assert grey(body).any() and (grey(body) | (body == 255).all(-1)).all(), "the wing alone: shaded grey on the background"
    with pytest.raises(ValueError, match="view takes"):
        env.render_frames_3d(size=SMALL, view=dict(elevation=10))
    env._reynolds_number = 123.0
    with pytest.raises(ValueError, match=r"123.*\[1000, 3000, 5000\]"):
        env.render_frames_3d(size=SMALL)
    env.close()


def test_a_2d_env_raises_and_an_unknown_reynolds_number_is_named():
    env = fluidgym_amd.make("ChannelJet2D-v0", num_envs=2, resolution_x=64, resolution_y=32)
    env.reset(seed=3)
    with pytest.raises(ValueError, match="2-D"):
        env.render_frames_3d()
    with pytest.raises(ValueError, match="2-D"):
        env.start_frame_recording(render_3d=True)
    assert env._frame_recorder is None
    env.close()
    env = fluidgym_amd.make("CylinderJet3D-easy-v0", num_envs=1, **CYL3)
    env.reset(seed=3)
    env._reynolds_number = 123.0
    with pytest.raises(ValueError, match=r"123.*\[100, 250, 500\]"):
        env.render_frames_3d(size=SMALL)
    env.close()


def test_parallel_env_forwards_frames_to_the_owning_lane():
    from fluidgym_amd.envs.parallel_env import ParallelFluidEnv

    kw = dict(n_heaters=2, resolution=4, use_marl=False, step_length=0.1, load_initial_domain=False, load_domain_statistics=False)
    env = ParallelFluidEnv("RBC3D-easy-v0", num_envs=4, lanes=2, **kw)
    try:
        env.reset(seed=5)
        lanes = env.lane_envs
        assert len(lanes) == 2 and lanes[0].num_envs == 2
        B = 4
        got = env.render_frames(envs=[0, B - 1])
        own = [lanes[0].render_frames(envs=[0]), lanes[1].render_frames(envs=[1])]
        assert list(got) == list(own[0])
        for key, t in got.items():
            assert t.shape[0] == 2 and torch.equal(t[0], own[0][key][0]) and torch.equal(t[1], own[1][key][0])
        got3 = env.render_frames_3d(envs=[B - 1, 0, 2], size=SMALL)["3d_temperature"]
        own3 = [lanes[1].render_frames_3d(envs=[1, 0], size=SMALL)["3d_temperature"], lanes[0].render_frames_3d(envs=[0], size=SMALL)["3d_temperature"]]
        assert tuple(got3.shape) == (3,) + SMALL + (3,)
        assert torch.equal(got3[0], own3[0][0]) and torch.equal(got3[1], own3[1][0]) and torch.equal(got3[2], own3[0][1])
        assert env.render_frames()["x-y-temperature"].shape[0] == B
        with pytest.raises(ValueError, match="this rank's batch"):
            env.render_frames(envs=[B])
    finally:
        env.close()
