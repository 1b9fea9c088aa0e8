"""``start_field_statistics`` / ``stop_field_statistics`` of the cylinder and airfoil envs: the record against a one-shot evaluation of
the fields the env went through, what is counted, that recording leaves the simulation untouched, and that the plane statistics
keep refusing a multi-block domain."""
import numpy as np
import pytest
import torch

import fluidgym_amd
from fluidgym_amd.simulation.cell_moments import CellMoments
from tests.cell_moments_ref import BOUND_ONE_SHOT, one_shot, worst_errors

pytestmark = pytest.mark.gpu

# the smallest meshes of tests/test_gpu_cylinder.py and tests/test_gpu_airfoil.py
KW = dict(resolution=8, initial_domain_steps=6, randomize_initial_state=False, step_length=0.05, dt=0.01, episode_length=3)
KW3 = dict(resolution=8, n_jets=4, initial_domain_steps=4, randomize_initial_state=False, step_length=0.03, dt=0.01, episode_length=2)
KW_AIRFOIL = dict(initial_domain_steps=6, randomize_initial_state=False, episode_length=3, resolution_div=4)
STEPS = 3


def _cylinder_run(every=None, **kw):
    """Three env steps of the 2-D jet cylinder under seeded random actions; ``every``: record (0 = once per env step)."""
    env = fluidgym_amd.make("CylinderJet2D-easy-v0", num_envs=2, **dict(KW, **kw))
    env.reset(seed=4)
    gen = torch.Generator().manual_seed(0)
    if every is not None:
        env.start_field_statistics(every=every or env._n_sim_steps)
    rewards, snapshots = [], []
    for _ in range(STEPS):
        a = (torch.rand(2, 1, generator=gen) * 2 - 1).to(env.cuda_device, env._dtype)
        rewards.append(env.step(a)[1].clone())
        snapshots.append((env._domain.velocity.clone(), env._domain.pressure.clone()))
    stats = env.stop_field_statistics() if every is not None else None
    sizes, sim_steps = [b.size for b in env._domain.blocks], env._n_sim_steps
    env.close()
    return stats, snapshots, rewards, sizes, sim_steps


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
def test_cylinder_record_equals_the_one_shot_over_the_fields_of_the_run(dtype):
    stats, snapshots, _, sizes, _ = _cylinder_run(every=0, dtype=dtype)
    assert snapshots[0][0].dtype == dtype and stats.samples == STEPS and stats.channels == ("u", "v", "p")
    em, ec = worst_errors(stats, one_shot(stats, [(u.cpu().numpy(), p.cpu().numpy()) for u, p in snapshots]))
    print(f"{dtype}: mean {em:.2e}, central {ec:.2e} of the absolute-monomial sum")
    assert em <= BOUND_ONE_SHOT and ec <= BOUND_ONE_SHOT
    for i, (nx, ny) in enumerate(sizes):
        assert stats.mean("u", i).shape == stats.covariance("u", "v", i).shape == stats.tke(i).shape == (2, ny, nx)
        assert stats.n(i) == float(STEPS) and np.all(stats.variance("p", i) >= 0.0)
    assert stats.flat("mean", "p").shape == (2, snapshots[0][1].shape[1])


def test_recording_leaves_the_run_bit_identical_and_counts_every_nth_step():
    stats, on, rewards_on, _, sim_steps = _cylinder_run(every=1)
    assert stats.samples == STEPS * sim_steps
    _, off, rewards_off, _, _ = _cylinder_run()
    assert torch.equal(on[-1][0], off[-1][0]) and torch.equal(on[-1][1], off[-1][1])
    assert all(torch.equal(a, b) for a, b in zip(rewards_on, rewards_off))
    assert _cylinder_run(every=2)[0].samples == (STEPS * sim_steps) // 2


def test_field_statistics_are_off_by_default_need_a_reset_and_the_plane_statistics_still_refuse():
    env = fluidgym_amd.make("CylinderJet2D-easy-v0", num_envs=2, **KW)
    assert env._hook("field_stats") is None
    with pytest.raises(RuntimeError, match="reset"):
        env.start_field_statistics()
    with pytest.raises(RuntimeError, match="no field statistics"):
        env.stop_field_statistics()
    env.reset(seed=4)
    assert env._hook("field_stats") is None
    with pytest.raises(RuntimeError, match="no field statistics"):
        env.stop_field_statistics()
    with pytest.raises(ValueError, match="at least 1"):
        env.start_field_statistics(every=0)
    with pytest.raises(NotImplementedError, match="single-block"):
        env.start_flow_statistics()
    env.start_field_statistics()
    assert isinstance(env.stop_field_statistics(), CellMoments) and env._hook("field_stats") is None
    env.close()


def test_cylinder3d_span_average_on_and_off():
    env = fluidgym_amd.make("CylinderJet3D-easy-v0", num_envs=2, **KW3)
    env.reset(seed=1)
    B, sizes = 2, [b.size for b in env._domain.blocks]
    # one env step recorded per cell, and the same samples into a span-averaged record beside it
    env.start_field_statistics(span_average=False)
    spanned = CellMoments.for_domain(env._domain, span_average=True)
    hook = env._step_hooks["field_stats"]
    record = hook.run
    hook.run = lambda: (record(), spanned.update(env._domain.velocity, env._domain.pressure))
    env.step(torch.zeros(env._zero_action.shape, device=env.cuda_device))
    cells = env.stop_field_statistics()
    assert cells.samples == spanned.samples == env._n_sim_steps and cells.channels == ("u", "v", "w", "p")
    for i, (nx, ny, nz) in enumerate(sizes):
        assert cells.n(i) == float(cells.samples) and spanned.n(i) == float(spanned.samples * nz)
        for ch in cells.channels:
            per_cell, column = cells.mean(ch, i), spanned.mean(ch, i)
            assert per_cell.shape == (B, nz, ny, nx) and column.shape == (B, ny, nx)
            # every sample has the same weight: the span average of the per-cell means is the mean of the column
            assert np.abs(per_cell.mean(axis=1) - column).max() <= 1e-12 * max(np.abs(per_cell).max(), 1e-30)
    # the env's own span-averaged record
    env.start_field_statistics()
    env.step(torch.zeros(env._zero_action.shape, device=env.cuda_device))
    stats = env.stop_field_statistics()
    for i, (nx, ny, nz) in enumerate(sizes):
        assert stats.n(i) == float(stats.samples * nz) and stats.tke(i).shape == (B, ny, nx) and np.isfinite(stats.tke(i)).all()
    env.close()


def test_airfoil_record_is_finite_and_gives_the_surface_pressure():
    env = fluidgym_amd.make("Airfoil2D-easy-v0", num_envs=2, **KW_AIRFOIL)
    env.reset(seed=0)
    env.start_field_statistics()
    env.step(0.3 * env.sample_action())
    stats = env.stop_field_statistics()
    assert stats.samples == env._n_sim_steps and len(stats.blocks) == len(env._domain.blocks)
    for i, blk in enumerate(env._domain.blocks):
        nx, ny = blk.size
        for ch in stats.channels:
            assert stats.mean(ch, i).shape == (2, ny, nx) and np.isfinite(stats.mean(ch, i)).all()
            assert np.isfinite(stats.variance(ch, i)).all() and np.all(stats.variance(ch, i) >= 0.0)
    surface = env._ring.cell_index                      # the wall-adjacent cells around the airfoil (2-D: a cell is a column)
    mean_p, var_p = stats.at_cells("p", surface)
    assert mean_p.shape == var_p.shape == (2, surface.numel()) and np.isfinite(mean_p).all() and np.all(var_p >= 0.0)
    assert np.array_equal(mean_p, stats.flat("mean", "p")[:, surface.cpu().numpy()])
    env.close()
