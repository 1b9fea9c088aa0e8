"""3-D frames, what holds without a GPU: the NumPy restatement of the ray marcher against geometry, the camera
convention, the closed forms of the volume mode, the library's exports and argument checks."""
import ctypes
import math

import numpy as np
import pytest
import torch

import fluidgym_amd  # noqa: F401
from fluidgym_amd import _lib as L
from fluidgym_amd.envs import frames as F
from fluidgym_amd.envs import render3d as R3

from tests import render3d_ref as R

f32 = np.float32
N, CENTRE, RADIUS = 33, 16.0, 10.0
H, W = 41, 37                      # the issue's image of 41 x 37 pixels
PIXEL = 0.9                        # cells per pixel: the image covers the 33-cell box


def sphere_volume():
    z, y, x = np.meshgrid(*(np.arange(N, dtype=np.float64),) * 3, indexing="ij")
    return np.sqrt((x - CENTRE) ** 2 + (y - CENTRE) ** 2 + (z - CENTRE) ** 2).astype(f32)[None, None]


def ortho_camera(direction, back=30.0):
    """Parallel unit-length rays along ``direction`` through the centre of the sphere volume, starting ``back`` cells before it."""
    d = np.asarray(direction, dtype=np.float64)
    d /= np.linalg.norm(d)
    helper = np.array([0.0, 1.0, 0.0]) if abs(d[1]) < 0.9 else np.array([1.0, 0.0, 0.0])
    right = np.cross(d, helper)
    right /= np.linalg.norm(right)
    down = np.cross(d, right)
    o0 = np.full(3, CENTRE) - back * d - 0.5 * W * PIXEL * right - 0.5 * H * PIXEL * down
    return R3.camera_from_vectors(o0, PIXEL * right, PIXEL * down, d, np.zeros(3), np.zeros(3)), back


def analytic(cam, back):
    """Distance of the centre from every ray and the depth of the analytic hit, from the camera's float32 entries in float64."""
    c = R3.camera_array(cam).astype(np.float64)
    pj, pi = np.arange(W) + 0.5, np.arange(H) + 0.5
    o = c[0][None, None] + pj[None, :, None] * c[1][None, None] + pi[:, None, None] * c[2][None, None]
    d = c[3] / np.linalg.norm(c[3])
    rel = np.full(3, CENTRE) - o
    along = rel @ d
    r = np.sqrt(np.maximum((rel ** 2).sum(-1) - along ** 2, 0.0))
    depth = along - np.sqrt(np.maximum(RADIUS ** 2 - r ** 2, 0.0))
    return r, depth, o, d


@pytest.fixture(scope="module")
def sphere_pictures():
    vol, table = sphere_volume(), F.resolve_colormap("rainbow")
    out = {}
    for name, direction in (("axis", (0.0, 0.0, 1.0)), ("oblique", (1.0, 2.0, 3.0))):
        cam, back = ortho_camera(direction)
        frames, depth, normal = R.isosurface(vol, 0, [RADIUS], vol, 0, [R.fixed_range(0.0, 20.0)], table, R3.camera_array(cam), H, W, 0.5,
                                             return_normal=True)
        out[name] = (cam, back, frames[0], depth[0], normal[0])
    return out


@pytest.mark.parametrize("name", ["axis", "oblique"])
def test_restatement_draws_the_analytic_sphere(sphere_pictures, name):
    """Bounds of the issue: outside a band of half a cell around the silhouette circle every pixel agrees on hit / no hit, the band
    leaves out at most 10 % of the pixels, the depth of the hits lies within a quarter cell of the analytic one (the method's own
    error, measured by a prototype: 7.3 % of the pixels in the band, no mismatch, depth error 0.072 cells)."""
    cam, back, frame, depth, _ = sphere_pictures[name]
    r, want, _, _ = analytic(cam, back)
    band = np.abs(r - RADIUS) <= 0.5
    hit = np.isfinite(depth)
    print(f"{name}: {band.mean():.3%} of the pixels in the band, {(hit != (r < RADIUS))[~band].sum()} mismatches, "
          f"depth error {np.abs(depth - want)[hit & ~band].max():.4f} cells")
    assert band.mean() <= 0.10
    assert np.array_equal(hit[~band], (r < RADIUS)[~band])
    assert np.abs(depth - want)[hit & ~band].max() <= 0.25
    assert (frame[~hit] == 255).all() and hit.sum() > 300            # the background is white, the disc is there


@pytest.mark.parametrize("name", ["axis", "oblique"])
def test_normal_points_outward_within_a_few_degrees(sphere_pictures, name):
    """Each component of the trilinear interpolant's gradient is a difference across the cell, i.e. the derivative of the distance
    field half-way along its own axis, up to half a cell from the hit: the direction errs by at most sqrt(3) 0.5 / 10 rad = 4.96
    degrees on a sphere of 10 cells; the bound is 5 degrees."""
    cam, back, _, depth, normal = sphere_pictures[name]
    r, _, o, d = analytic(cam, back)
    hit = np.isfinite(depth) & (r < RADIUS - 0.5)
    point = o[hit] + depth[hit][:, None].astype(np.float64) * R3.camera_array(cam).astype(np.float64)[3][None]
    radial = (point - CENTRE) / np.linalg.norm(point - CENTRE, axis=1, keepdims=True)
    n = normal[hit].astype(np.float64)
    cosine = (n * radial).sum(1) / np.linalg.norm(n, axis=1)
    print(f"{name}: largest angle between normal and radius {np.degrees(np.arccos(np.clip(cosine.min(), -1, 1))):.2f} degrees")
    assert cosine.min() >= math.cos(math.radians(5.0))


VIEWS = [(15, 60), (10, 60), (15, 45), (15, 0), (15, 90), (15, 180), (15, 270)]      # the families' default views, then the cardinal ones


@pytest.mark.parametrize("projection", ["persp", "ortho"])
@pytest.mark.parametrize("elev,azim", VIEWS)
def test_marker_corner_lands_in_the_quadrant_the_convention_names(elev, azim, projection):
    """The written convention (envs/render3d.py): the viewer stands at (-cos e cos a, sin e, cos e sin a), y points up, so the image's
    right is sin(a) x + cos(a) z: at azim 0 +z is right, at 90 +x, at 180 -z, at 270 -x.  A bright blob in one corner of an otherwise
    empty box must show in the quadrant this names."""
    nz, ny, nx = 11, 9, 13
    table = F.resolve_colormap("viridis")
    cam = R3.orbit_camera((nz, ny, nx), (2.6, 1.8, 2.2), elev, azim, size=(24, 32), projection=projection)
    for sx, sy, sz in ((1, 1, 1), (-1, 1, -1), (1, -1, 1), (-1, -1, -1)):
        vol = np.zeros((1, 1, nz, ny, nx), f32)
        vol[0, 0, (slice(-4, -1) if sz > 0 else slice(1, 4)), (slice(-4, -1) if sy > 0 else slice(1, 4)), (slice(-4, -1) if sx > 0 else slice(1, 4))] = 1.0
        frames, depth = R.isosurface(vol, 0, [0.5], vol, 0, [R.fixed_range(0, 1)], table, R3.camera_array(cam), 24, 32, R3.default_step(cam))
        rows, cols = np.nonzero(np.isfinite(depth[0]))
        assert rows.size >= 4, (sx, sy, sz)
        want_right = sx * math.sin(math.radians(azim)) + sz * math.cos(math.radians(azim)) > 0
        assert (cols.mean() > 16.0) == want_right, (sx, sy, sz, cols.mean())
        assert (rows.mean() < 12.0) == (sy > 0), (sx, sy, sz, rows.mean())


def test_perspective_and_orthographic_cameras_share_the_centre_ray():
    for elev, azim in VIEWS:
        cams = [R3.camera_array(R3.orbit_camera((20, 30, 40), (4.0, 2.0, 1.0), elev, azim, size=(48, 64), projection=p)).astype(np.float64)
                for p in ("persp", "ortho")]
        o, d = [c[0] + 32 * c[1] + 24 * c[2] for c in cams], [c[3] + 32 * c[4] + 24 * c[5] for c in cams]
        assert np.allclose(o[0], o[1], rtol=0, atol=1e-4) and np.allclose(d[0], d[1], rtol=0, atol=1e-5)
        assert not cams[0][1:3].any() and not cams[1][4:6].any()            # persp: ou = ov = 0; ortho: du = dv = 0
        centre = 0.5 * (np.array([40, 30, 20]) - 1.0)
        t = ((centre - o[0]) * d[0]).sum() / (d[0] * d[0]).sum()
        assert np.allclose(o[0] + t * d[0], centre, atol=1e-3)                # the centre ray goes through the centre of the box


def _along_x_camera(shape, Hh, Ww):
    nz, ny, nx = shape
    return R3.camera_from_vectors((-2.0, 0.0, 0.0), (0, (ny - 1) / Ww, 0), (0, 0, (nz - 1) / Hh), (1, 0, 0), (0, 0, 0), (0, 0, 0))


def test_volume_mode_closed_forms():
    shape, Hh, Ww = (5, 6, 40), 4, 5
    cam = R3.camera_array(_along_x_camera(shape, Hh, Ww))
    table = F.resolve_colormap("rainbow")
    const = np.full((1, 1) + shape, 0.5, f32)
    rng = [R.fixed_range(0.0, 1.0)]
    k = int(math.floor(39 / 0.5)) + 1                                         # samples of a ray through the box along x
    a = 0.005
    frames, alpha = R.volume(const, 0, rng, table, np.full(256, a, f32), cam, Hh, Ww, 0.5, return_alpha=True)
    closed = 1.0 - (1.0 - float(f32(a))) ** k
    assert closed < 0.99 and np.abs(alpha.astype(np.float64) - closed).max() <= 4 * k * 2.0 ** -24
    colour = table[128].astype(np.float64)
    want = np.floor(closed * colour + (1 - closed) * 255.0 + 0.5)
    assert np.abs(frames[0].astype(np.float64) - want[None, None]).max() <= 1
    # zero opacity: the background; full opacity: the colour of the first sample (a ramp along x starts in bin 0)
    background = (10, 20, 30)
    frames = R.volume(const, 0, rng, table, np.zeros(256, f32), cam, Hh, Ww, 0.5, background=background)
    assert (frames == np.array(background, np.uint8)).all()
    ramp = np.broadcast_to(np.linspace(0, 1, shape[2], dtype=f32), (1, 1) + shape).copy()
    frames, alpha = R.volume(ramp, 0, rng, table, np.ones(256, f32), cam, Hh, Ww, 0.5, background=background, return_alpha=True)
    assert (frames == table[0]).all() and (alpha == 1).all()
    # a ray that misses the box shows the background
    away = R3.camera_array(R3.camera_from_vectors((-2, 50, 0), (0, 0, 0), (0, 0, 0), (1, 0, 0), (0, 0, 0), (0, 0, 0)))
    assert (R.volume(ramp, 0, rng, table, np.ones(256, f32), away, 2, 2, 0.5, background=background) == np.array(background, np.uint8)).all()


def test_log_opacity_table():
    t = R3.log_opacity_table(0.05)
    assert t.dtype == np.float32 and t.shape == (256,) and np.all(np.diff(t) > 0) and 0 < t[0] < t[-1] < 0.05
    assert abs(t[-1] - 0.05 * math.log1p(255.5 / 256) / math.log(2)) < 1e-8
    assert not R3.log_opacity_table(0.0).any()
    with pytest.raises(ValueError, match="strength"):
        R3.log_opacity_table(1.5)


def test_library_exports_the_ray_marcher_in_the_fp32_build_only():
    for name in ("fg_render_isosurface", "fg_render_volume"):
        assert hasattr(L.load(), name) and name in L.SIGNATURES
        assert name not in L.SIGNATURES_F64 and not hasattr(L.load_f64(), name)
    header = open(fluidgym_amd.__file__.replace("fluidgym_amd/__init__.py", "include/fluidgym_hip.h")).read()
    assert "int fg_render_isosurface(" in header and "int fg_render_volume(" in header and "} fg_render_camera;" in header
    assert ctypes.sizeof(L.FgRenderCamera) == 72 and ctypes.sizeof(L.FgRenderOptions) == 48
    assert [n for n, _ in L.FgRenderCamera._fields_] == ["o0", "ou", "ov", "d0", "du", "dv"]


def test_argument_checks_answer_before_any_launch():
    """Every check of the two entries answers FG_ERR_INVALID_ARG with a message, on a machine without a GPU: the pointers below are host
    arrays the library must never get to read (only envs, the camera and the options, which are host data by contract)."""
    lib = L.load()
    B, C, nz, ny, nx = 3, 2, 4, 5, 6
    vol = np.zeros((B, C, nz, ny, nx), f32)
    table, rng, level, opacity = np.zeros((256, 3), np.uint8), np.zeros((2, 2), f32), np.zeros(2, f32), np.zeros(256, f32)
    out = np.zeros((2, 4, 4, 3), np.uint8)
    envs = np.array([2, 0], np.int32)
    good_cam = ((0, 0, -3), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0), (0, 0, 0))

    def call(entry, shape=(B, C, nz, ny, nx), channel=0, cchannel=0, cam=good_cam, step=0.5, clip=None, size=(4, 4), envs_=envs, n=2, null=()):
        camera = R3.camera_from_vectors(*cam)
        opt = R3._options(step, camera, clip, (128, 128, 128), (255, 255, 255))
        ptr = lambda name, a: None if name in null else ctypes.c_void_p(a.ctypes.data)
        cam_p = None if "camera" in null else ctypes.byref(camera)
        opt_p = None if "options" in null else ctypes.byref(opt)
        env_p = None if "envs" in null else envs_.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        if entry == "fg_render_isosurface":
            rc = lib.fg_render_isosurface(ptr("volume", vol), *shape, channel, ptr("level", level), ptr("color_volume", vol), C, cchannel,
                                          ptr("range", rng), ptr("table", table), None, cam_p, opt_p, *size, env_p, n, ptr("out", out), None, None)
        else:
            rc = lib.fg_render_volume(ptr("volume", vol), *shape, channel, ptr("range", rng), ptr("table", table), ptr("opacity", opacity),
                                      cam_p, opt_p, *size, env_p, n, ptr("out", out), None)
        return rc, lib.fg_last_error().decode()

    nulls = {"fg_render_isosurface": ("volume", "level", "color_volume", "range", "table", "camera", "options", "envs", "out"),
             "fg_render_volume": ("volume", "range", "table", "opacity", "camera", "options", "envs", "out")}
    bad_d0 = lambda v: good_cam[:3] + (v,) + good_cam[4:]
    cases = [
        (dict(n=0), "n must be"),
        (dict(shape=(B, C, nz, 1, nx)), "extent"),
        (dict(shape=(B, C, 1, ny, nx)), "at least 2"),
        (dict(envs_=np.array([0, 3], np.int32)), "envs[1] = 3"),
        (dict(envs_=np.array([-1, 0], np.int32)), "envs[0] = -1"),
        (dict(channel=2), "channel 2"),
        (dict(channel=-2), "channel -2"),
        (dict(size=(0, 4)), "H and W"),
        (dict(size=(4, 0)), "H and W"),
        (dict(size=(32768, 32768)), "2^31 bytes"),
        (dict(step=0.0), "step"),
        (dict(step=-1.0), "step"),
        (dict(step=float("nan")), "step"),
        (dict(cam=bad_d0((0, 0, 0))), "d0 is zero"),
        (dict(cam=bad_d0((0, float("nan"), 1))), "non-finite"),
        (dict(cam=bad_d0((float("inf"), 0, 1))), "non-finite"),
    ]
    for entry in nulls:
        for name in nulls[entry]:
            rc, msg = call(entry, null=(name,))
            assert rc == L.FG_ERR_INVALID_ARG and "null" in msg and msg.startswith(entry), (entry, name, msg)
        for kw, needle in cases:
            rc, msg = call(entry, **kw)
            assert rc == L.FG_ERR_INVALID_ARG and needle in msg and msg.startswith(entry), (entry, kw, msg)
    for kw, needle in [(dict(clip=((0, 3, 0), (5, 2, 3))), "clip box is empty along axis y"), (dict(cchannel=2), "colour channel 2"),
                       (dict(cchannel=-2), "colour channel -2")]:
        rc, msg = call("fg_render_isosurface", **kw)
        assert rc == L.FG_ERR_INVALID_ARG and needle in msg and msg.startswith("fg_render_isosurface"), (kw, msg)
    assert not out.any()
    # the Python doors refuse a view that is not on the GPU: there is no CPU path
    cam = R3.orbit_camera((4, 4, 4), (1, 1, 1), 15, 60, size=(4, 4))
    with pytest.raises(L.NativeLibraryError, match="no CPU path"):
        R3.raycast_isosurface(torch.zeros(1, 1, 4, 4, 4), 0, 0.5, torch.zeros(1, 1, 4, 4, 4), 0, (0, 1), "viridis", cam)
    with pytest.raises(L.NativeLibraryError, match="no CPU path"):
        R3.raycast_volume(torch.zeros(1, 1, 4, 4, 4), 0, (0, 1), "viridis", R3.log_opacity_table(), cam)


def test_orbit_camera_refuses_bad_arguments():
    ok = dict(shape=(4, 5, 6), extent=(1.0, 2.0, 3.0), elev=15, azim=60)
    assert R3.orbit_camera(**ok, size=(3, 5)).size == (3, 5)
    for kw, needle in [(dict(projection="fisheye"), "projection"), (dict(size=(0, 5)), "size"), (dict(size=(5, -1)), "size"),
                       (dict(extent=(1.0, 0.0, 3.0)), "extent"), (dict(extent=(1.0, 2.0)), "extent"), (dict(extent=(1.0, float("nan"), 1.0)), "extent"),
                       (dict(shape=(4, 1, 6)), "at least 2"), (dict(up_axis="w"), "up_axis"), (dict(zoom=0.0), "zoom")]:
        with pytest.raises(ValueError, match=needle):
            R3.orbit_camera(**{**ok, **kw})
    # looking straight down the up axis still has a right: the azimuth names it
    assert np.isfinite(R3.camera_array(R3.orbit_camera(**{**ok, "elev": 90}))).all()


def test_camera_keeps_its_image_size_and_the_recorder_takes_the_3d_size():
    import copy

    cam = R3.orbit_camera((4, 5, 6), (1.0, 2.0, 3.0), 15, 60, size=(3, 5))
    assert isinstance(cam, L.FgRenderCamera) and ctypes.sizeof(cam) == 18 * 4                 # the library's struct as it stands
    twin = copy.copy(cam)
    assert twin.size == (3, 5) and np.array_equal(R3.camera_array(twin), R3.camera_array(cam))
    assert R3.default_step(twin) == R3.default_step(cam)
    by_hand = R3.camera_from_vectors((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0), (0, 0, 0))
    assert by_hand.size is None and R3.default_step(by_hand) == 0.5
    assert F.FrameRecorder([0], 1, 24).size_3d is None and F.FrameRecorder([0], 1, 24, size_3d=[24, 32]).size_3d == (24, 32)
