"""``start_flow_statistics`` / ``stop_flow_statistics`` of the TCF and RBC envs: what is counted, that the friction velocity of the
record is the wall stress the env reports, and that recording leaves the simulation untouched."""
import numpy as np
import pytest
import torch

import fluidgym_amd

pytestmark = pytest.mark.gpu

TCF = dict(num_envs=2, randomize_initial_state=False, resolution_x_z=16, resolution_y=16, step_length=0.6, use_marl=False)
STEPS = 3


def _tcf_run(record: bool):
    env = fluidgym_amd.make("TCFSmall3D-both-easy-v0", **TCF)
    env.reset(seed=4)
    gen = torch.Generator().manual_seed(0)
    if record:
        env.start_flow_statistics(order=4)
    tau = []
    for _ in range(STEPS):
        a = (torch.rand(env._zero_action.shape, generator=gen) * 2 - 1).to(env.cuda_device)
        tau.append(env.step(a)[4]["wall_stress"].double().cpu().numpy())
    stats = env.stop_flow_statistics() if record else None
    state = (env._block.velocity.clone(), env._block.pressure.clone())
    sim_steps = env._n_sim_steps
    env.close()
    return stats, np.mean(tau, axis=0), state, sim_steps


def test_tcf_statistics_count_match_the_wall_stress_and_leave_the_state_alone():
    stats, tau, state, sim_steps = _tcf_run(True)
    assert stats.channels == ("u", "v", "w", "p") and stats.order == 4
    assert stats.n.tolist() == [float(STEPS * sim_steps * 16 * 16)] * 2
    uw2 = stats.u_wall() ** 2
    print("u_wall^2", uw2, "mean wall stress", tau, "relative difference", np.abs(uw2 - tau) / tau)
    assert np.all(np.abs(uw2 - tau) <= 1e-5 * tau)
    assert stats.mean("u").shape == (2, 16) and np.isfinite(stats.moment_standardized("u", 4)).all()
    assert np.all(stats.Re_wall() > 0) and stats.half_channel().mean("u").shape == (2, 8)
    _, tau_off, state_off, _ = _tcf_run(False)
    assert torch.equal(state[0], state_off[0]) and torch.equal(state[1], state_off[1])
    assert np.array_equal(tau, tau_off)


def test_statistics_are_off_by_default_and_need_a_reset():
    env = fluidgym_amd.make("TCFSmall3D-both-easy-v0", **TCF)
    assert env._hook("flow_stats") is None
    with pytest.raises(RuntimeError, match="reset"):
        env.start_flow_statistics()
    with pytest.raises(RuntimeError, match="no statistics"):
        env.stop_flow_statistics()
    env.reset(seed=4)
    env.start_flow_statistics(order=2, every=2)
    env.step(torch.zeros(env._zero_action.shape, device=env.cuda_device))
    stats = env.stop_flow_statistics()
    assert env._hook("flow_stats") is None and stats.n.tolist() == [float((env._n_sim_steps // 2) * 16 * 16)] * 2
    env.close()


def test_rbc2d_records_the_temperature():
    env = fluidgym_amd.make("RBC2D-easy-v0", num_envs=2, n_heaters=4, resolution=8, randomize_initial_state=False, step_length=0.5)
    env.reset(seed=1)
    env.start_flow_statistics(order=3)
    for _ in range(2):
        env.step(torch.zeros(2, 4, 1, device="cuda"))
    stats = env.stop_flow_statistics()
    ny, nx = env._block.velocity.shape[-2:]
    assert stats.channels == ("u", "v", "p", "T")
    assert stats.n.tolist() == [float(2 * env._n_sim_steps * nx)] * 2
    T = stats.mean("T")
    print("mean temperature profile of env 0:", T[0])
    assert T.shape == (2, ny) and np.all(T >= 0.0) and np.all(T <= 1.0)
    assert np.all(stats.variance("T") >= 0.0) and np.isfinite(stats.pooled().moment_standardized("T", 3)).all()
    env.close()
