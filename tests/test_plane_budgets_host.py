"""Reynolds-stress budgets without a GPU: ``HostPlaneBudgets`` in zero-border mode against the reference's golden values (means,
second-order sums and the terms made of them) and against a long-double one-shot evaluation (third-order sums, turbulent
transport, both border modes), the second difference of ``viscous_diffusion``, pooling, the half-channel fold, files, and the ABI of
``fg_plane_budgets``."""
import ctypes
import os
import re

import numpy as np
import pytest

from fluidgym_amd import _lib as L
from fluidgym_amd.simulation.plane_budgets import (FILE_GRAD, FILE_MOMENTS, BudgetRecord, HostPlaneBudgets, PlaneBudgets, budget_keys,
                                                   central_gradient, channel_names)
from tests.plane_budgets_ref import (BOUND_GOLDEN, BOUND_ONE_SHOT, channel_stack, make_grid, make_samples, one_shot, worst_errors)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_plane_budgets.npz")
PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1))
ZERO = (False, False)


def _run(samples, grid, forcing, wrap):
    acc = HostPlaneBudgets(*grid, forcing=forcing, wrap=wrap)
    for u, p, s in samples:
        acc.update(u, p, s)
    return acc


def _golden_run(g, forcing):
    grid = (g["x"], g["y"], g["z"])
    samples = [(g["velocity"][s], g["pressure"][s], g["source"][s]) for s in range(3)]
    return _run(samples, grid, forcing, ZERO), one_shot([channel_stack(s, grid, forcing, ZERO) for s in samples], forcing)


def _ref_key(key, forcing):
    """The reference's name of a central sum: exponents over its own channels (u, v, w, dp/dx_j (, s_j)) or, for a gradient
    record, over (d_k u, d_k v, d_k w); with the index of the gradient record or None."""
    if key[0] >= 6 and key[0] < 15:
        k = (key[0] - 6) // 3
        chans = [6 + 3 * k + i for i in range(3)]
    else:
        k, chans = None, list(range(6)) + ([15, 16, 17] if forcing else [])
    return k, "_".join(str(sum(1 for c in key if c == ch)) for ch in chans)


def test_keys_and_channels():
    for forcing, K, M in ((False, 15, 43), (True, 18, 52)):
        keys = budget_keys(forcing)
        assert len(keys) == M == len(set(keys)) and len(channel_names(forcing)) == K
        assert all(tuple(sorted(k)) == k and max(k) < K for k in keys)
        assert [len(k) for k in keys].count(3) == 10
    assert budget_keys(False)[:7] == [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2), (0, 0, 0)]


@pytest.mark.parametrize("forcing", [False, True])
def test_means_and_second_order_sums_equal_the_reference_golden_values(forcing):
    g = np.load(GOLDEN)
    pre = "f_" if forcing else "nf_"
    acc, truth = _golden_run(g, forcing)
    n, _, _, abs1, absM = truth
    assert acc.n.tolist() == [float(g[pre + "n"])] == [3.0 * 4 * 6]
    _, mean, cen = acc._state()
    worst = 0.0
    for c in range(acc.K):
        if c < 6 or c >= 15:
            ref = g[pre + "mean_%d" % (c if c < 6 else c - 9)][:, :, 0]
        else:
            ref = g[pre + "grad%d_mean_%d" % ((c - 6) // 3, (c - 6) % 3)][:, :, 0]
        worst = max(worst, np.max(np.abs(mean[..., c] - ref) / np.asarray(abs1[..., c] / n[:, None], np.float64)))
    seen = 0
    for q, key in enumerate(acc.keys):
        if len(key) != 2:
            continue
        k, name = _ref_key(key, forcing)
        ref = g[pre + ("moment_" if k is None else "grad%d_moment_" % k) + name][:, :, 0]
        worst = max(worst, np.max(np.abs(cen[..., q] - ref) / np.asarray(absM[..., q], np.float64)))
        seen += 1
    assert seen == acc.M - 10
    print("worst error against the golden values / absolute-monomial sum:", worst)
    assert worst <= BOUND_GOLDEN
    # the terms made of means and second-order sums: relative to the largest value of the reference's profile
    terms = ["production", "dissipation", "velocity_pressure_gradient"] + (["velocity_forcing"] if forcing else [])
    for t in terms:
        for i, j in PAIRS:
            ref = g[pre + "%s_%d%d" % (t, i, j)]
            err = np.max(np.abs(getattr(acc, t)(i, j)[0] - ref)) / np.max(np.abs(ref))
            print(t, i, j, "error / largest term:", err)
            assert err <= BOUND_GOLDEN, (t, i, j, err)
    if not forcing:
        with pytest.raises(RuntimeError, match="Forcing"):
            acc.velocity_forcing(0, 0)


@pytest.mark.parametrize("forcing", [False, True])
def test_third_order_sums_and_turbulent_transport_equal_the_one_shot_on_the_golden_inputs(forcing):
    g = np.load(GOLDEN)
    acc, truth = _golden_run(g, forcing)
    em, ec = worst_errors(acc, truth)
    print(f"forcing {forcing}: mean {em:.2e}, central {ec:.2e} of the absolute-monomial sum")
    assert em <= BOUND_ONE_SHOT and ec <= BOUND_ONE_SHOT
    n, _, cen, _, absM = truth
    for i, j in PAIRS:
        q = acc._index[tuple(sorted((i, j, 1)))]
        exact = -central_gradient(np.asarray(cen[..., q] / n[:, None], np.float64), g["y"], 1)
        scale = np.max(np.abs(central_gradient(np.asarray(absM[..., q] / n[:, None], np.float64), g["y"], 1)))
        assert np.max(np.abs(acc.turbulent_transport(i, j) - exact)) <= BOUND_ONE_SHOT * scale


@pytest.mark.parametrize("forcing", [False, True])
@pytest.mark.parametrize("wrap", [ZERO, (True, True), (True, False)])
def test_merged_samples_pooled_and_merge_equal_the_one_shot(forcing, wrap):
    shape = (2, 5, 6, 7)
    grid = make_grid(*shape[1:])
    samples = make_samples(shape, seed=11, dtype=np.float64)
    acc = _run(samples, grid, forcing, wrap)
    stacks = [channel_stack(s, grid, forcing, wrap) for s in samples]
    em, ec = worst_errors(acc, one_shot(stacks, forcing))
    print(f"forcing {forcing} wrap {wrap}: mean {em:.2e}, central {ec:.2e} of the absolute-monomial sum")
    assert em <= BOUND_ONE_SHOT and ec <= BOUND_ONE_SHOT
    pm, pc = worst_errors(acc.pooled(), one_shot(stacks, forcing, pool_envs=True))
    print(f"pooled: mean {pm:.2e}, central {pc:.2e}")
    assert pm <= BOUND_ONE_SHOT and pc <= BOUND_ONE_SHOT
    a, b = _run(samples[:1], grid, forcing, wrap), _run(samples[1:], grid, forcing, wrap)
    mm, mc = worst_errors(a.merge(b), one_shot(stacks, forcing))
    assert mm <= BOUND_ONE_SHOT and mc <= BOUND_ONE_SHOT
    with pytest.raises(ValueError, match="same"):
        a.merge(_run(samples[:1], grid, forcing, (not wrap[0], wrap[1])))


def test_wrap_differs_from_zero_only_in_the_border_columns():
    shape = (1, 4, 5, 6)
    grid = make_grid(*shape[1:])
    u, p, s = make_samples(shape, samples=1, seed=2, dtype=np.float64)[0]
    from fluidgym_amd.simulation.plane_budgets import budget_channels
    cz, cw = budget_channels(u, p, None, *grid, wrap=ZERO), budget_channels(u, p, None, *grid, wrap=(True, True))
    for c in range(15):
        same = cz[c] == cw[c]
        if c in (3, 6, 7, 8):                 # d/dx
            assert same[..., 1:-1].all() and not same[..., 0].any() and not same[..., -1].any()
        elif c in (5, 12, 13, 14):            # d/dz
            assert same[:, 1:-1].all() and not same[:, 0].any() and not same[:, -1].any()
        else:
            assert same.all()
    # on a periodic field the wrapped difference at the seam is the interior one
    wave = np.sin(2 * np.pi * np.arange(6) / 6.0).reshape(1, 1, 1, 1, 6) * np.ones((1, 3, 4, 5, 1))
    gx = budget_channels(wave, p, None, *grid, wrap=(True, True))[6]
    assert np.allclose(gx[0, 0, 0], (np.roll(wave[0, 0, 0, 0], -1) - np.roll(wave[0, 0, 0, 0], 1)) / (2 * 0.37), rtol=1e-14)


def test_viscous_diffusion_is_the_second_derivative_on_a_non_uniform_grid():
    """<u'u'> = y^2 on rows whose coordinates are dyadic rationals, so that every operation is exact: 2 on interior rows."""
    y = np.array([0.125, 0.25, 0.5, 1.0, 1.25, 2.0, 2.5])
    rec = HostPlaneBudgets([0.0, 1.0], y, [0.0, 1.0])
    cen = np.zeros((1, len(y), rec.M))
    cen[0, :, rec._index[(0, 0)]] = 4.0 * y ** 2
    rec._set_state(np.array([4.0]), np.zeros((1, len(y), rec.K)), cen)
    vd = rec.viscous_diffusion(0, 0)
    assert vd.shape == (1, len(y)) and np.array_equal(vd[0, 1:-1], np.full(len(y) - 2, 2.0))
    assert not rec.viscous_diffusion(1, 1).any()
    # wall units: lengths by nu / u_wall, velocities by u_wall
    rec.set_wall_units(np.linspace(-0.9, 0.9, len(y)), 0.5)
    mean = np.zeros((1, len(y), rec.K))
    mean[0, :, 0] = 1.0 - np.linspace(-0.9, 0.9, len(y)) ** 2
    rec._set_state(np.array([4.0]), mean, cen)
    uw = rec.u_wall()
    assert np.allclose(uw ** 2, 0.5 * 0.19 / 0.1, rtol=1e-14)
    assert np.allclose(rec.viscous_diffusion(0, 0, as_wall=True), vd * (0.5 / uw[:, None] ** 2) ** 2, rtol=1e-14)
    assert np.allclose(rec.covariance(0, 0, as_wall=True), rec.covariance(0, 0) / uw[:, None] ** 2, rtol=1e-14)
    b = rec.budget(0, 0)
    assert set(b) == {"production", "dissipation", "turbulent_transport", "viscous_diffusion", "velocity_pressure_gradient"}
    assert np.array_equal(b["viscous_diffusion"], 0.5 * vd)
    assert np.allclose(rec.residual(0, 0), sum(v for k, v in b.items() if k != "dissipation") - b["dissipation"], rtol=1e-15)
    assert np.allclose(rec.residual(0, 0, as_wall=True), rec.residual(0, 0) * 0.5 / uw[:, None] ** 4, rtol=1e-12, atol=1e-12)


def test_accessors_are_the_reference_formulas_of_the_record():
    shape = (2, 3, 6, 4)
    grid = make_grid(*shape[1:])
    acc = _run(make_samples(shape, seed=3, dtype=np.float64), grid, True, (True, True))
    n, mean, cen = acc._state()
    norm = lambda key: cen[..., acc._index[key]] / n[:, None]
    assert acc.mean(2).shape == (2, 6) and np.array_equal(acc.mean(2), mean[..., 2])
    assert np.array_equal(acc.mean_grad(0, 1), mean[..., 9]) and not acc.mean_grad(0, 0).any() and not acc.mean_grad(1, 2).any()
    assert np.array_equal(acc.covariance(1, 0), norm((0, 1))) and np.array_equal(acc.skewness(2, 0, 1), norm((0, 1, 2)))
    assert np.array_equal(acc.covariance_grad(2, 0, 1), norm((9, 11)))
    assert np.array_equal(acc.production(0, 1), -norm((0, 1)) * mean[..., 10] - norm((1, 1)) * mean[..., 9])
    assert np.array_equal(acc.dissipation(0, 0), 2.0 * ((norm((6, 6)) + norm((9, 9))) + norm((12, 12))))
    assert np.array_equal(acc.velocity_pressure_gradient(0, 1), -(norm((0, 4)) + norm((1, 3))))
    assert np.array_equal(acc.velocity_forcing(0, 2), norm((0, 17)) + norm((2, 15)))
    assert np.array_equal(acc.turbulent_transport(0, 0), -central_gradient(norm((0, 0, 1)), grid[1], 1))
    with pytest.raises(RuntimeError, match="viscosity"):
        acc.budget(0, 0)
    with pytest.raises(RuntimeError, match="wall units"):
        acc.mean(0, as_wall=True)
    with pytest.raises(IndexError):
        acc.covariance(0, 3)
    with pytest.raises(KeyError):
        acc.central_sum((3, 3))
    with pytest.raises(ValueError, match="monotonic"):
        HostPlaneBudgets([0.0, 0.0], grid[1], grid[2])
    with pytest.raises(ValueError, match="2-D"):
        HostPlaneBudgets(*grid).update(np.zeros((1, 2, 6, 4)), np.zeros((1, 1, 6, 4)))
    with pytest.raises(ValueError, match="source"):
        HostPlaneBudgets(*grid, forcing=True).update(np.zeros((1, 3, 3, 6, 4)), np.zeros((1, 1, 3, 6, 4)))
    with pytest.raises(ValueError, match="GPU"):
        PlaneBudgets(*grid).update(np.zeros((1, 3, 3, 6, 4)), np.zeros((1, 1, 3, 6, 4)))


def test_a_non_finite_cell_poisons_its_row_and_the_two_next_to_it():
    shape = (2, 3, 6, 7)
    grid = make_grid(*shape[1:])
    samples = make_samples(shape, seed=5, dtype=np.float64)
    clean = _run(samples, grid, False, (True, True))
    samples[1][0][1, 1, 1, 3, 4] = np.nan           # sample 1, env 1, channel v, z 1, y 3, x 4
    dirty = _run(samples, grid, False, (True, True))
    bad = np.zeros((2, 6), bool)
    bad[1, 2:5] = True
    for a, b in zip(clean._state()[1:], dirty._state()[1:]):
        assert np.isnan(b[bad]).all() and np.array_equal(a[~bad], b[~bad])
    assert np.array_equal(clean.n, dirty.n)


def test_half_channel_of_a_field_and_its_mirror_is_symmetric():
    """A sample and its mirror image (y -> -y, v -> -v, s_y -> -s_y) on rows symmetric about 0: the record is symmetric under the
    fold, which therefore returns the lower rows with every cell counted twice."""
    shape = (1, 3, 6, 5)
    grid = make_grid(*shape[1:])
    grid = (grid[0], 0.5 * (grid[1] - grid[1][::-1]), grid[2])          # symmetric about 0 to the last bit
    u, p, s = make_samples(shape, samples=1, seed=8, dtype=np.float64)[0]
    flip = np.array([1.0, -1.0, 1.0]).reshape(1, 3, 1, 1, 1)
    mirror = (u[:, :, :, ::-1] * flip, p[:, :, :, ::-1], s[:, :, :, ::-1] * flip)
    acc = _run([(u, p, s), mirror], grid, True, (True, True)).set_wall_units(grid[1], 0.1)
    half = acc.half_channel()
    n, mean, cen = acc._state()
    hn, hm, hc = half._state()
    assert hm.shape == (1, 3, 18) and np.array_equal(hn, 2 * n) and np.array_equal(half.y, grid[1][:3])
    stacks = [channel_stack(sm, grid, True, (True, True)) for sm in ((u, p, s), mirror)]
    _, _, _, abs1, absM = one_shot(stacks, True)
    em = np.abs(hm - mean[:, :3]) / np.asarray(abs1[:, :3] / n[:, None, None], np.float64)
    ec = np.abs(hc - 2.0 * cen[:, :3]) / np.asarray(2 * absM[:, :3], np.float64)
    print("fold of a symmetric record: mean", em.max(), "central", ec.max())
    assert em.max() <= BOUND_ONE_SHOT and ec.max() <= BOUND_ONE_SHOT
    # and the record itself is symmetric: row y equals the mirrored row with the parity of each channel
    from fluidgym_amd.simulation.plane_budgets import _PARITY
    assert np.max(np.abs(mean[:, ::-1] * np.array(_PARITY) - mean) / np.asarray(abs1 / n[:, None, None], np.float64)) <= BOUND_ONE_SHOT
    assert np.array_equal(half._u_wall_fixed, acc.u_wall())
    assert half.production(0, 1, as_wall=True).shape == (1, 3)


@pytest.mark.parametrize("forcing", [False, True])
def test_save_writes_the_reference_key_names_and_load_returns_the_same_bits(tmp_path, forcing):
    g = np.load(GOLDEN)
    pre = "f_" if forcing else "nf_"
    shape = (3, 4, 6, 8)
    grid = make_grid(*shape[1:])
    acc = _run(make_samples(shape, seed=7), grid, forcing, (True, False)).set_wall_units(grid[1], 1.0 / 3.0)
    acc.save(tmp_path / "per_env")
    acc.save(tmp_path / "pooled", pooled=True)
    back = BudgetRecord.load(tmp_path / "per_env")
    for a, b in zip(acc._state(), back._state()):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    assert back.forcing == forcing and back.wrap == (True, False) and back.viscosity == acc.viscosity
    assert all(np.array_equal(a, b) for a, b in zip((back.x, back.y, back.z, back.y_centers), grid + (grid[1],)))
    pooled = BudgetRecord.load(tmp_path / "pooled")
    for a, b in zip(acc.pooled()._state(), pooled._state()):
        assert a.tobytes() == b.tobytes()
    for d in (tmp_path / "pooled", tmp_path / "per_env" / "env_0002"):
        assert sorted(f for f in os.listdir(d) if f.endswith(".npz")) == sorted([FILE_MOMENTS] + [FILE_GRAD % k for k in range(3)])
        with np.load(d / FILE_MOMENTS) as z:
            assert sorted(z.keys()) == list(g[pre + "keys_moments"])
            assert int(z["channels"]) == (9 if forcing else 6) and z["mean_000003"].shape == (1, 6, 1) and z["n"] == 3 * 4 * 8 * (3 if d.name == "pooled" else 1)
        for k in range(3):
            with np.load(d / (FILE_GRAD % k)) as z:
                assert sorted(z.keys()) == list(g[pre + "keys_grad_0001"])
    with np.load(tmp_path / "per_env" / "env_0001" / (FILE_GRAD % 2)) as z:
        assert np.array_equal(z["moment_1_0_1"][0, :, 0], acc.central_sum((12, 14))[1])
    with np.load(tmp_path / "per_env" / "env_0001" / FILE_MOMENTS) as z:
        assert np.array_equal(z["moment_1_1_1" + "_0" * (6 if forcing else 3)][0, :, 0], acc.central_sum((0, 1, 2))[1])
        assert np.array_equal(z["moment_0_1_0_0_0_1" + ("_0_0_0" if forcing else "")][0, :, 0], acc.central_sum((1, 5))[1])


def test_plane_budgets_abi():
    header = open(os.path.join(ROOT, "include", "fluidgym_hip.h")).read()
    assert re.search(r"\bint\s+fg_plane_budgets\s*\(", header)
    assert "fg_plane_budgets" in L.SIGNATURES and "fg_plane_budgets" in L.SIGNATURES_F64
    mk = open(os.path.join(ROOT, "fluidgym_amd", "csrc", "Makefile")).read()
    assert all("fg_planebudgets.hip" in line for line in mk.splitlines() if line.startswith(("SRCS =", "F64_SRCS =")))
    if not (os.path.exists(L.LIB_PATH) and os.path.exists(L.LIB_F64_PATH)):
        return
    one = ctypes.c_void_p(64)          # never dereferenced: every call below fails its argument checks first
    ptrs = (ctypes.c_void_p * 7)(*([64] * 7))
    holes = (ctypes.c_void_p * 7)(64, 64, None, 64, 64, 64, 64)
    late_hole = (ctypes.c_void_p * 7)(64, 64, 64, 64, 64, None, 64)
    strides = (ctypes.c_int64 * 7)(*([8] * 7))
    short = (ctypes.c_int64 * 7)(8, 8, 8, 7, 8, 8, 8)
    for lib in (L.load(), L.load_f64()):
        f = lib.fg_plane_budgets
        ok = (one, one, one, 1, 1, one, one, one, one)                      # x, y, z, wrap_x, wrap_z, n, mean, central, tickets
        bad = [(None, strides, 4, 1, 2, 2, 2) + ok, (ptrs, None, 4, 1, 2, 2, 2) + ok,            # null tables
               (holes, strides, 4, 1, 2, 2, 2) + ok, (late_hole, strides, 7, 1, 2, 2, 2) + ok,   # a null field
               (ptrs, strides, 5, 1, 2, 2, 2) + ok, (ptrs, strides, 3, 1, 2, 2, 2) + ok,         # n_fields neither 4 nor 7
               (ptrs, strides, 4, 0, 2, 2, 2) + ok,                                              # batch
               (ptrs, strides, 4, 1, 1, 2, 2) + ok, (ptrs, strides, 4, 1, 2, 1, 2) + ok, (ptrs, strides, 4, 1, 2, 2, 1) + ok,   # nz, ny, nx = 1
               (ptrs, short, 4, 1, 2, 2, 2) + ok, (ptrs, strides, 7, 1, 2, 2, 3) + ok]           # a batch stride below nz * ny * nx
        for pos in (0, 1, 2, 5, 6, 7, 8):                                                        # null coordinates / accumulators
            bad.append((ptrs, strides, 7, 1, 2, 2, 2) + ok[:pos] + (None,) + ok[pos + 1:])
        for args in bad:
            assert f(*args, None) == -1, args
            assert b"fg_plane_budgets" in lib.fg_last_error()
