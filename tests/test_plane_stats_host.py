"""Plane-averaged flow statistics without a GPU: ``HostPlaneMoments`` against the reference's golden values (order 2) and against a
long-double one-shot evaluation (every order), pooling, files, wall units, and the ABI of ``fg_plane_moments``."""
import ctypes
import os
import re

import numpy as np
import pytest

from fluidgym_amd import _lib as L
from fluidgym_amd.simulation.plane_stats import (FILE_COV, FILE_MOMENTS, FILE_P, FILE_VEL, HostPlaneMoments, PlaneMoments,
                                                 merge_moments, moment_keys)
from tests.plane_stats_ref import BOUND_GOLDEN, BOUND_ONE_SHOT, channel_stack, make_samples, one_shot, worst_errors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_plane_stats.npz")
PROBE = (2, 9, 5, 130)        # sheared mean profile, three samples: the shape the merge rules were probed at


def _run(samples, K, order, channels=None):
    acc = HostPlaneMoments(channels or {3: ("u", "v", "p"), 4: ("u", "v", "w", "p"), 5: ("u", "v", "w", "p", "T")}[K], order)
    for u, p, T in samples:
        acc.update(u, p, T)
    return acc


def test_order_two_equals_the_reference_golden_values():
    g = np.load(GOLDEN)
    acc = HostPlaneMoments(("u", "v", "w", "p"), 2)
    for s in range(3):
        acc.update(g["velocity"][s], g["pressure"][s])
    stacks = [np.concatenate([g["velocity"][s][:, c][None] for c in range(3)] + [g["pressure"][s][:, 0][None]]) for s in range(3)]
    n, mean, cen, abs1, absM = one_shot(stacks, 2)
    assert acc.n.tolist() == [float(g["vel_n"])] == [float(g["mom_n"])] == [float(g["cov_n"])] == [float(g["p_n"])]
    worst = 0.0
    for c in range(4):        # means: the Welford classes [1, C, Y] and the moments class [1, Y, 1]
        ref = g["vel_mean"][:, c] if c < 3 else g["p_mean"][:, 0]
        scale = np.asarray(abs1[..., c] / n[:, None], np.float64)
        worst = max(worst, np.max(np.abs(acc.mean(c) - ref) / scale), np.max(np.abs(acc.mean(c) - g["mom_mean_%d" % c][:, :, 0]) / scale))
    for q, key in enumerate(moment_keys(4, 2)):
        scale = np.asarray(absM[..., q], np.float64)
        refs = [g["mom_moment_" + "_".join(map(str, key))][:, :, 0]]
        if max(key) == 2:
            c = key.index(2)
            refs.append(g["vel_sum_squares"][:, c] if c < 3 else g["p_sum_squares"][:, 0])
        if key == (1, 1, 0, 0):
            refs.append(g["cov_C"][:, 0])
        for ref in refs:
            worst = max(worst, np.max(np.abs(acc.moment(key) - ref) / scale))
    print("worst error against the golden values / absolute-monomial sum:", worst)
    assert worst <= BOUND_GOLDEN
    assert np.array_equal(acc.variance("u"), acc.moment((2, 0, 0, 0)) / 120.0)
    assert np.array_equal(acc.covariance("u", "v"), acc.covariance(1, 0))


@pytest.mark.parametrize("K,order", [(4, 2), (4, 3), (4, 4), (5, 4), (3, 4)])
def test_merged_samples_equal_the_one_shot(K, order):
    shape = PROBE if K != 3 else (2, 1, 5, 130)
    samples = make_samples(shape, K, seed=11, dtype=np.float64)
    acc = _run(samples, K, order)
    stacks = [channel_stack(s, K) for s in samples]
    em, ec = worst_errors(acc, one_shot(stacks, order))
    print(f"K {K} order {order}: mean {em:.2e}, central {ec:.2e} of the absolute-monomial sum")
    assert em <= BOUND_ONE_SHOT and ec <= BOUND_ONE_SHOT
    # pooled(): all envs and samples as one ensemble
    pm, pc = worst_errors(acc.pooled(), one_shot(stacks, order, pool_envs=True))
    print(f"pooled: mean {pm:.2e}, central {pc:.2e}")
    assert pm <= BOUND_ONE_SHOT and pc <= BOUND_ONE_SHOT
    # merge(): two records of disjoint samples are the record of all of them
    a, b = _run(samples[:1], K, order), _run(samples[1:], K, order)
    mm, mc = worst_errors(a.merge(b), one_shot(stacks, order))
    assert mm <= BOUND_ONE_SHOT and mc <= BOUND_ONE_SHOT


def test_accessors_and_standardized_moments():
    samples = make_samples((2, 4, 6, 32), 4, seed=3, dtype=np.float64)
    acc = _run(samples, 4, 4)
    n, mean, cen, _, _ = one_shot([channel_stack(s, 4) for s in samples], 4)
    assert acc.mean("p").shape == (2, 6) and acc.n.shape == (2,)
    assert np.array_equal(acc.moment((0, 0, 0, 0)), np.full((2, 6), 3 * 4 * 32.0)) and not acc.moment((0, 1, 0, 0)).any()
    m2, m3, m4 = (np.asarray(cen[..., acc._index[acc._pure("u", o)]] / n[:, None], np.float64) for o in (2, 3, 4))
    assert np.allclose(acc.moment_standardized("u", 3), m3 / m2 ** 1.5, rtol=1e-10, atol=0)
    assert np.allclose(acc.moment_standardized("u", 4), m4 / m2 ** 2, rtol=1e-10, atol=0)
    assert np.array_equal(acc.moment_normalized((0, 0, 0, 2)), acc.variance("p"))
    with pytest.raises(KeyError):
        acc.moment((2, 1, 0, 0))
    with pytest.raises(KeyError):
        _run(samples, 4, 2).moment((3, 0, 0, 0))
    with pytest.raises(ValueError):
        HostPlaneMoments(("u", "p"))
    with pytest.raises(ValueError):
        HostPlaneMoments(order=5)
    with pytest.raises(ValueError, match="multi-block"):
        HostPlaneMoments().update(np.zeros((1, 3, 40)), np.zeros((1, 1, 40)))
    with pytest.raises(ValueError, match="GPU"):
        PlaneMoments().update(*samples[0][:2])


def test_a_non_finite_cell_poisons_its_row_only():
    samples = make_samples((2, 3, 5, 7), 4, seed=5, dtype=np.float64)
    clean = _run(samples, 4, 3)
    samples[1][0][1, 2, 1, 3, 4] = np.nan           # sample 1, env 1, channel w, z 1, y 3, x 4
    dirty = _run(samples, 4, 3)
    bad = np.zeros((2, 5), bool)
    bad[1, 3] = True
    for a, b in zip(clean._state()[1:], dirty._state()[1:]):
        assert np.isnan(b[bad]).all() and np.array_equal(a[~bad], b[~bad])
    assert np.array_equal(clean.n, dirty.n)


def test_save_load_round_trip_and_reference_key_names(tmp_path):
    g = np.load(GOLDEN)
    samples = make_samples((3, 4, 6, 8), 4, seed=7)
    acc = _run(samples, 4, 2).set_wall_units(np.linspace(-0.9, 0.9, 6), 1.0 / 3.0)
    acc.save(tmp_path / "per_env")
    acc.save(tmp_path / "pooled", pooled=True)
    back = HostPlaneMoments.load(tmp_path / "per_env")
    for a, b in zip(acc._state(), back._state()):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    assert back.channels == acc.channels and back.order == 2 and back.viscosity == acc.viscosity
    assert np.array_equal(back.y_centers, acc.y_centers)
    pooled = HostPlaneMoments.load(tmp_path / "pooled")
    for a, b in zip(acc.pooled()._state(), pooled._state()):
        assert a.tobytes() == b.tobytes()
    for d in (tmp_path / "pooled", tmp_path / "per_env" / "env_0002"):
        for name, keys in ((FILE_VEL, "keys_welford"), (FILE_P, "keys_welford"), (FILE_COV, "keys_covariance"), (FILE_MOMENTS, "keys_moments")):
            with np.load(d / name) as z:
                assert sorted(z.keys()) == list(g[keys]), (name, sorted(z.keys()))
    with np.load(tmp_path / "per_env" / "env_0001" / FILE_VEL) as z:      # the layouts of the reference's arrays
        assert z["mean"].shape == g["vel_mean"].shape[:2] + (6,) and z["n"] == 3 * 4 * 8
        assert np.array_equal(z["mean"][0, 2], acc.mean("w")[1]) and np.array_equal(z["sum_squares"][0, 1], acc.moment((0, 2, 0, 0))[1])
    with np.load(tmp_path / "per_env" / "env_0001" / FILE_COV) as z:
        assert z["C"].shape == (1, 1, 6) and np.array_equal(z["C"][0, 0], acc.moment((1, 1, 0, 0))[1])
    with np.load(tmp_path / "per_env" / "env_0001" / FILE_MOMENTS) as z:
        assert z["mean_000003"].shape == (1, 6, 1) == g["mom_mean_3"].shape[:1] + (6, 1)
    # order 4 files hold the pure third- and fourth-order sums under the same naming
    _run(samples, 4, 4).save(tmp_path / "o4", pooled=True)
    with np.load(tmp_path / "o4" / FILE_MOMENTS) as z:
        assert {"moment_3_0_0_0", "moment_0_0_0_4"} <= set(z.keys()) and int(z["num_moments"]) == 18


def test_wall_units_and_half_channel_fold():
    """A laminar profile u = 1 - y^2 between walls at -1 and 1, v antisymmetric: u_wall from the wall rows, the fold merges
    mirrored rows with the sign of v flipped."""
    ny, nu = 8, 0.01
    e = np.linspace(-1, 1, ny + 1)
    y = 0.5 * (e[1:] + e[:-1])
    rng = np.random.default_rng(1)
    acc = HostPlaneMoments(("u", "v", "w", "p"), 3).set_wall_units(y, nu)
    stacks = []
    for s in range(2):
        f = 0.05 * rng.standard_normal((4, 1, 3, ny, 16))
        f[0] += (1 - y ** 2).reshape(1, 1, ny, 1)
        f[1] += (0.1 * y).reshape(1, 1, ny, 1)
        acc.update(np.moveaxis(f[:3], 0, 1), np.moveaxis(f[3:], 0, 1))
        stacks.append(f)
    u = acc.mean("u")
    tau = nu * 0.5 * (u[:, 0] / (1 + y[0]) + u[:, -1] / (1 - y[-1]))
    assert np.allclose(acc.u_wall() ** 2, tau, rtol=1e-15) and np.allclose(acc.Re_wall(), acc.u_wall() / nu, rtol=1e-15)
    assert np.allclose(acc.to_wall_pos(y)[0], (y + 1) * acc.u_wall()[0] / nu) and acc.to_wall_pos(y).shape == (1, ny)
    assert np.allclose(acc.to_wall_vel(acc.variance("u"), 2), acc.variance("u") / acc.u_wall()[:, None] ** 2)
    half = acc.half_channel()
    # the same thing in one shot: the mirrored upper half with v negated, appended as further cells of the lower rows
    folded = []
    for f in stacks:
        up = f[:, :, :, ::-1][:, :, :, :ny // 2].copy()
        up[1] *= -1
        folded += [f[:, :, :, :ny // 2], up]
    em, ec = worst_errors(half, one_shot(folded, 3))
    assert em <= BOUND_ONE_SHOT and ec <= BOUND_ONE_SHOT and half.mean("u").shape == (1, ny // 2)
    assert np.array_equal(half.y_centers, y[:ny // 2])


def test_merge_moments_with_an_empty_side_returns_the_other():
    rng = np.random.default_rng(2)
    m, c = rng.standard_normal((2, 3, 4)), rng.standard_normal((2, 3, 18))
    n = np.full((2, 1), 40.0)
    for out in (merge_moments(np.zeros((2, 1)), m * np.nan, c * np.nan, n, m, c, 4, 4), merge_moments(n, m, c, np.zeros((2, 1)), m * 0, c * 0, 4, 4)):
        assert np.array_equal(out[0], n) and np.array_equal(out[1], m) and np.array_equal(out[2], c)


def test_plane_moments_abi():
    header = open(os.path.join(ROOT, "include", "fluidgym_hip.h")).read()
    assert re.search(r"\bint\s+fg_plane_moments\s*\(", header)
    assert "fg_plane_moments" in L.SIGNATURES and "fg_plane_moments" in L.SIGNATURES_F64
    assert not "fg_plane_moments".startswith(L._F64_ABSENT_PREFIXES)
    mk = open(os.path.join(ROOT, "fluidgym_amd", "csrc", "Makefile")).read()
    assert all("fg_planestats.hip" in line for line in mk.splitlines() if line.startswith(("SRCS =", "F64_SRCS =")))
    one = ctypes.c_void_p(64)          # never dereferenced: every call below fails its argument checks first
    ptrs = (ctypes.c_void_p * 5)(*([64] * 5))
    holes = (ctypes.c_void_p * 5)(64, 64, None, 64, 64)
    strides = (ctypes.c_int64 * 5)(*([8] * 5))
    short = (ctypes.c_int64 * 5)(8, 8, 7, 8, 8)
    for lib in (L.load(), L.load_f64()):
        f = lib.fg_plane_moments
        bad = [
            (None, strides, 4, 1, 1, 2, 4, 2, one, one, one, one),        # null tables
            (ptrs, None, 4, 1, 1, 2, 4, 2, one, one, one, one),
            (holes, strides, 4, 1, 1, 2, 4, 2, one, one, one, one),       # a null channel
            (ptrs, strides, 4, 1, 1, 2, 4, 2, None, one, one, one),       # null accumulators
            (ptrs, strides, 4, 1, 1, 2, 4, 2, one, None, one, one),
            (ptrs, strides, 4, 1, 1, 2, 4, 2, one, one, None, one),
            (ptrs, strides, 4, 1, 1, 2, 4, 2, one, one, one, None),
            (ptrs, strides, 2, 1, 1, 2, 4, 2, one, one, one, one),        # K outside 3..5
            (ptrs, strides, 6, 1, 1, 2, 4, 2, one, one, one, one),
            (ptrs, strides, 4, 1, 1, 2, 4, 1, one, one, one, one),        # order outside 2..4
            (ptrs, strides, 4, 1, 1, 2, 4, 5, one, one, one, one),
            (ptrs, strides, 4, 0, 1, 2, 4, 2, one, one, one, one),        # non-positive extents
            (ptrs, strides, 4, 1, 0, 2, 4, 2, one, one, one, one),
            (ptrs, strides, 4, 1, 1, -2, 4, 2, one, one, one, one),
            (ptrs, strides, 4, 1, 1, 2, 0, 2, one, one, one, one),
            (ptrs, short, 4, 1, 1, 2, 4, 2, one, one, one, one),          # a batch stride below nz * ny * nx
        ]
        for args in bad:
            assert f(*args, None) == -1, args
            assert b"fg_plane_moments" in lib.fg_last_error()
