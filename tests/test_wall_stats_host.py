"""Wall distributions and their statistics without a GPU: the NumPy twin of the device function against the reference's golden
forces and its exact properties, ``HostWallMoments`` against a long-double one-shot evaluation, merging, pooling and the file, the
geometry ``WallRing`` adds on a host-built cylinder mesh, the separation points, and the argument checks of both entry points."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from fluidgym_amd import _lib as L
from fluidgym_amd.envs.surface import ring_chord_coordinates, ring_theta, separation_points
from fluidgym_amd.simulation.wall_stats import CHANNELS, HostWallMoments, WallRecord, sample_wall_faces
from tests.wall_stats_ref import BOUND_ONE_SHOT, bad_argument_lists, make_fields, make_ring, one_shot, worst_errors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "reference_forces.npz"))


def _golden_geom():
    return np.stack([G["normals"][0], G["normals"][1], G["tangent_lengths"], G["dist"], G["face_len"]])


def test_twin_integrates_to_the_reference_forces():
    """fx, fy times the face length, summed over the ring, is the force tests/test_forces.py pins on the reference's function; per
    layer in 3-D."""
    n = G["p"].shape[0]
    idx = np.arange(n)[None]
    d = sample_wall_faces(G["u_cell"][None], G["u_b"][None], G["p"][None], idx, idx, _golden_geom(), float(G["nu"][0]), np.float64)
    assert d.shape == (1, 4, 1, n) and d.dtype == np.float64
    f = (d[0, 2:4, 0] * G["face_len"]).sum(-1)
    assert np.allclose(f, G["force"], rtol=1e-10)
    assert np.array_equal(d[0, 0, 0], G["p"])
    nz = G["p3"].shape[0]
    idx3 = np.arange(nz * n).reshape(nz, n)
    d3 = sample_wall_faces(G["u3"].reshape(1, 3, -1), G["ub3"].reshape(1, 3, -1), G["p3"].reshape(1, -1), idx3, idx3, _golden_geom(),
                           float(G["nu"][0]), np.float64)
    assert d3.shape == (1, 4, nz, n)
    f3 = (d3[0, 2:4] * G["areas"]).sum(-1)                    # [2, nz]
    assert np.allclose(f3, G["force3"], rtol=1e-10)
    # a per-env viscosity is the scalar of that env
    two = sample_wall_faces(np.repeat(G["u_cell"][None], 2, 0), np.repeat(G["u_b"][None], 2, 0), np.repeat(G["p"][None], 2, 0), idx, idx,
                            _golden_geom(), np.array([float(G["nu"][0]), 0.5]), np.float64)
    assert np.array_equal(two[0], d[0]) and not np.array_equal(two[1, 1], d[0, 1])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_fluid_at_the_wall_velocity_feels_the_pressure_only(dtype):
    """A uniform velocity equal to the wall's: every gradient is zero, so the traction is -p n and the shear stress 0, exactly."""
    ci, si, geom, N, NB = make_ring(67, 3, seed=1, dtype=dtype)
    _, _, p = make_fields(2, 2, N, NB, seed=1, dtype=dtype)
    u, ub = np.empty((2, 2, N), dtype), np.empty((2, 2, NB), dtype)
    for c, val in enumerate((0.7, -0.3)):
        u[:, c], ub[:, c] = val, val
    d = sample_wall_faces(u, ub, p, ci, si, geom, 0.01, dtype)
    pc = p[:, ci]
    assert d.dtype == dtype and np.array_equal(d[:, 0], pc)
    assert np.array_equal(d[:, 1], np.zeros_like(pc))
    assert np.array_equal(d[:, 2], -pc * geom[0]) and np.array_equal(d[:, 3], -pc * geom[1])


def test_a_pressure_constant_shifts_the_normal_traction_only():
    """p + c: channel 0 moves by c, fx, fy by -c n (to rounding: p enters them by one subtraction), tau_w not by a bit."""
    ci, si, geom, N, NB = make_ring(67, 3, seed=2, dtype=np.float64)
    u, ub, p = make_fields(2, 2, N, NB, seed=2, dtype=np.float64)
    c = 3.0
    a, scale = sample_wall_faces(u, ub, p, ci, si, geom, 0.01, np.float64, with_scale=True)
    b = sample_wall_faces(u, ub, p + c, ci, si, geom, 0.01, np.float64)
    assert np.array_equal(b[:, 0], (p + c)[:, ci])
    assert a[:, 1].tobytes() == b[:, 1].tobytes()
    tol = 16 * np.finfo(np.float64).eps * (scale + c)
    assert np.all(np.abs(b[:, 2] - (a[:, 2] - c * geom[0])) <= tol[:, 2]) and np.all(np.abs(b[:, 3] - (a[:, 3] - c * geom[1])) <= tol[:, 3])
    assert np.all(scale >= np.abs(a))


def _samples(n, layers, B, count, seed):
    ci, si, geom, N, NB = make_ring(n, layers, seed=seed, dtype=np.float64)
    return [sample_wall_faces(*make_fields(B, 2, N, NB, seed=seed, dtype=np.float64, sample=s), ci, si, geom, 0.01, np.float64)
            for s in range(count)]


def _run(samples, span_average):
    acc = HostWallMoments(samples[0].shape[3], samples[0].shape[2], span_average)
    for s in samples:
        acc.update(s)
    return acc


@pytest.mark.parametrize("span_average", [True, False])
def test_host_moments_merge_pooled_and_file_equal_the_one_shot(span_average, tmp_path):
    samples = _samples(19, 3, B=3, count=5, seed=4)
    acc = _run(samples, span_average)
    assert acc.samples == 5 and acc.count == (15.0 if span_average else 5.0) and acc.R == (19 if span_average else 57)
    em, ec = worst_errors(acc, one_shot(samples, span_average))
    print(f"span_average={span_average}: mean {em:.2e}, central {ec:.2e} of the absolute-monomial sum")
    assert em <= BOUND_ONE_SHOT and ec <= BOUND_ONE_SHOT
    # two halves merged are the whole
    a, b = _run(samples[:2], span_average), _run(samples[2:], span_average)
    mm, mc = worst_errors(a.merge(b), one_shot(samples, span_average))
    assert mm <= BOUND_ONE_SHOT and mc <= BOUND_ONE_SHOT and a.samples == 5
    empty = HostWallMoments(19, 3, span_average)
    assert empty.merge(b).samples == 3 and np.array_equal(empty._state()[0], b._state()[0])
    with pytest.raises(ValueError, match="same ring"):
        a.merge(HostWallMoments(19, 3, not span_average))
    # the envs pooled: every env's faces in one record
    pooled = acc.pooled()
    truth = one_shot([s[e:e + 1] for s in samples for e in range(3)], span_average)
    pm, pc = worst_errors(pooled, truth)
    print(f"pooled: mean {pm:.2e}, central {pc:.2e}")
    assert pm <= BOUND_ONE_SHOT and pc <= BOUND_ONE_SHOT and pooled.samples == 15
    # accessors
    shape = (3, 19) if span_average else (3, 3, 19)
    assert acc.mean("tau_w").shape == shape and acc.channels == CHANNELS
    assert np.array_equal(acc.variance("fx"), acc.covariance("fx", "fx")) and np.array_equal(acc.covariance(0, 3), acc.covariance("fy", "p"))
    assert np.allclose(acc.rms("p") ** 2, acc.variance("p"), rtol=1e-14) and np.all(acc.variance("p") >= 0)
    with pytest.raises(RuntimeError, match="no sample"):
        HostWallMoments(19, 3).mean("p")
    with pytest.raises(ValueError):
        acc.update(samples[0][:, :, :2])
    # the file
    acc.save(tmp_path / "wall.npz")
    back = WallRecord.load(tmp_path / "wall.npz")
    assert back.samples == 5 and (back.n_faces, back.layers, back.span_average) == (19, 3, span_average)
    for x, y in zip(acc._state(), back._state()):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes()


def test_one_layer_first_sample_is_the_distribution_itself():
    s = _samples(7, 1, B=2, count=1, seed=6)[0]
    acc = _run([s], True)
    assert acc._state()[0].tobytes() == s[:, :, 0].tobytes() and not acc._state()[1].any()


def test_wall_ring_curve_geometry_on_a_host_built_cylinder_mesh():
    from fluidgym_amd.envs.cylinder_grid import BOTTOM, LEFT, RIGHT, TOP, build_domain, make_vortex_street_mesh
    from fluidgym_amd.envs.forces import WallRing
    from tests import stub_mb

    restore = stub_mb.install()
    try:
        dom = build_domain(make_vortex_street_mesh(8), 0.01, batch=1, device="cpu")
        ring = WallRing(dom, [(LEFT, "+x", False), (TOP, "-y", False), (RIGHT, "-x", True), (BOTTOM, "+y", True)])
    finally:
        restore()
    n = ring.n_faces
    v = ring.vertices.numpy()
    fl = np.sqrt(((v[:, 1:] - v[:, :-1]) ** 2).sum(0))
    assert n == 32 and ring.face_centers.shape == (2, n) and ring.arc_length.shape == (n,)
    assert np.allclose(v[:, 0], v[:, -1], atol=1e-12)                                 # a closed ring
    assert np.isclose(ring.arc_length[-1] + fl[-1] / 2, fl.sum(), rtol=1e-14)
    assert np.all(np.diff(ring.arc_length) > 0) and np.isclose(ring.arc_length[0], fl[0] / 2, rtol=1e-14)
    assert np.array_equal(ring.face_centers, 0.5 * (v[:, 1:] + v[:, :-1]))
    # theta: strictly monotone along the ring apart from one wrap, inside (-180, 180]
    theta = ring_theta(ring.face_centers, v)
    assert theta.shape == (n,) and np.all(theta > -180.0) and np.all(theta <= 180.0)
    steps = np.diff(np.concatenate([theta, theta[:1]]))                               # cyclic: the closing step included
    direction = np.sign(np.median(steps))
    assert direction != 0 and np.count_nonzero(np.sign(steps) != direction) == 1
    assert np.all(np.abs(steps[np.sign(steps) == direction]) < 360.0 / n * 1.5)
    # the upstream-most face midpoint is the one nearest theta = 0
    c = v[:, :-1].mean(axis=1)
    assert np.argmin(np.abs(theta)) == np.argmin(ring.face_centers[0] - 1e-9 * np.abs(ring.face_centers[1] - c[1]))
    # counter-clockwise from upstream: theta = +90 degrees is the lowest point of the ring
    assert np.argmin(np.abs(theta - 90.0)) in np.argsort(ring.face_centers[1])[:2]
    # the midpoints lie inside the circle of radius D / 2 by no more than the polygon's sagitta
    r = np.sqrt(((v[:, :-1] - c[:, None]) ** 2).sum(0))
    assert np.allclose(r, 0.5, rtol=1e-5)
    depth = 0.5 - np.sqrt(((ring.face_centers - c[:, None]) ** 2).sum(0))
    sagitta = 0.5 - np.sqrt(0.25 - (fl / 2) ** 2)
    assert np.all(depth >= -1e-6) and np.all(depth <= sagitta + 1e-6)
    # the tables the kernels share
    ci, si, geom = ring.native_tables(torch.float64)
    assert ci.dtype == torch.int32 and tuple(ci.shape) == tuple(si.shape) == (1, n) and tuple(geom.shape) == (5, n) and geom.dtype == torch.float64
    assert ring.native_tables(torch.float64)[2] is geom and ring.native_tables()[0] is ci and ring.native_tables()[2].dtype == torch.float32
    assert ring._native[2] is ring.native_tables()[2]
    # the airfoil coordinates of the same ring: x / c in [0, 1], the side from the normal
    x_over_c, side = ring_chord_coordinates(ring.face_centers, v, ring.wall_normals.numpy())
    assert x_over_c.min() > 0 and x_over_c.max() < 1 and set(side) == {1.0, -1.0}
    assert np.array_equal(side > 0, ring.wall_normals.numpy()[1] >= 0)


def test_separation_points_on_hand_made_sign_patterns():
    s, per = np.array([0.5, 1.5, 2.5, 3.5]), 4.0
    got = separation_points(np.array([[1.0, 1.0, -1.0, -1.0],          # between faces 1 and 2, and across the wrap (3 -> 0)
                                      [-1.0, 3.0, 1.0, 3.0],           # faces 0 | 1 at a quarter, wrap at three quarters of its step
                                      [2.0, 1.0, 0.5, 3.0],            # no crossing
                                      [-2.0, -1.0, -0.5, -3.0],
                                      [1.0, -1.0, -1.0, -1.0]]), s, per)
    assert [len(g) for g in got] == [2, 2, 0, 0, 2]
    assert np.allclose(got[0], [0.0, 2.0], atol=1e-15) and np.allclose(got[1], [0.25, 0.75], atol=1e-15)
    assert np.allclose(got[4], [0.0, 1.0], atol=1e-15)
    one = separation_points(torch.tensor([1.0, -3.0, -1.0, -1.0]), torch.as_tensor(s), per)      # one env, tensors
    assert len(one) == 1 and np.allclose(one[0], [0.0, 0.75])
    # a face at exactly zero counts as positive: the crossing sits on it
    assert np.allclose(separation_points(np.array([1.0, 0.0, -1.0, 1.0]), s, per)[0], [1.5, 3.0])
    with pytest.raises(ValueError):
        separation_points(np.zeros((2, 3)), s, per)


def test_wall_stats_abi_and_argument_checks():
    """Both libraries declare, type and build the two entries, and the argument checks return before anything touches the device."""
    header = open(os.path.join(ROOT, "include", "fluidgym_hip.h")).read()
    mk = open(os.path.join(ROOT, "fluidgym_amd", "csrc", "Makefile")).read()
    assert all("fg_wallstats.hip" in line for line in mk.splitlines() if line.startswith(("SRCS =", "F64_SRCS =")))
    assert re.search(r"^fg_wallstats\.o \$\(F64_DIR\)/fg_wallstats\.o: CXXFLAGS \+= -ffp-contract=off$", mk, flags=re.M)
    for name in ("fg_mb_wall_distribution", "fg_mb_wall_moments"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header)
        assert name in L.SIGNATURES and name in L.SIGNATURES_F64
        assert L.SIGNATURES[name][1][12] is ctypes.c_float and L.SIGNATURES_F64[name][1][12] is ctypes.c_double
    for lib in (L.load(), L.load_f64()):
        for name, moments in (("fg_mb_wall_distribution", False), ("fg_mb_wall_moments", True)):
            cases = bad_argument_lists(moments)
            assert len(cases) >= 20
            for args in cases:
                assert getattr(lib, name)(*args, None) == -1, (name, args)
                assert name.encode() in lib.fg_last_error()


def test_envs_without_a_wall_ring_refuse():
    import fluidgym_amd
    from fluidgym_amd.envs.parallel_env import ParallelFluidEnv

    env = fluidgym_amd.make("RBC2D-easy-v0", cuda_device="cpu")
    with pytest.raises(NotImplementedError, match="wall ring"):
        env.get_surface_distribution()
    with pytest.raises(NotImplementedError, match="ParallelFluidEnv"):
        ParallelFluidEnv.get_surface_distribution(None)
