"""``start_flow_time_correlation`` / ``stop_flow_time_correlation`` of the TCF and RBC envs: what the schedule counts, that lag 0
is 1 and nothing exceeds it, that the lag times are those of the simulation's clock, and that recording leaves the simulation
untouched."""
import numpy as np
import pytest
import torch

import fluidgym_amd

pytestmark = pytest.mark.gpu

TCF = dict(num_envs=2, randomize_initial_state=False, resolution_x_z=16, resolution_y=16, step_length=0.6, use_marl=False)
STEPS = 3


def _tcf_run(record: bool, every: int = 1):
    env = fluidgym_amd.make("TCFSmall3D-both-easy-v0", **TCF)
    env.reset(seed=4)
    gen = torch.Generator().manual_seed(0)
    n = env._n_sim_steps
    if record:
        env.start_flow_time_correlation(lags=2 * n, every=every, stride=n)
    tau = []
    for _ in range(STEPS):
        a = (torch.rand(env._zero_action.shape, generator=gen) * 2 - 1).to(env.cuda_device)
        tau.append(env.step(a)[4]["wall_stress"].double().cpu().numpy())
    corr = env.stop_flow_time_correlation() if record else None
    state = (env._block.velocity.clone(), env._block.pressure.clone())
    sim = env._sim
    dt = sim.time_step * (1 if sim.substeps == -1 else max(sim.substeps, 1))
    u_wall, nu = env._u_wall, env._nu
    env.close()
    return corr, np.mean(tau, axis=0), state, n, dt, (u_wall, nu)


def test_tcf_correlations_follow_the_schedule_and_leave_the_state_alone():
    corr, tau, state, n, dt, (u_wall, nu) = _tcf_run(True)
    assert corr.channels == ("u", "v", "w") and corr.lags == 2 * n and corr.n_slots == 2 and corr.samples == STEPS * n
    # bases at the samples 0, n, 2 n of 3 n: all three reach the lags below n, the first two the lags from n on
    assert corr.count.tolist() == [3.0] * n + [2.0] * n
    for c in corr.channels:
        coef = corr.coefficient(c)
        assert coef.shape == (2, 16, 2 * n)
        print(c, "coefficient at the largest lag, env 0:", coef[0, :, -1])
        assert np.abs(coef[..., 0] - 1.0).max() <= 1e-6 and np.abs(coef).max() <= 1.0 + 1e-6
        assert np.abs(corr.correlation(c)).max() <= 1.0 + 1e-6 and np.isfinite(corr.integral_time(c)).all()
    want = dt * np.arange(2 * n)
    assert np.abs(corr.lag_time() - want[None]).max() <= 1e-12 * want[-1]
    assert np.allclose(corr.lag_ETT(), corr.lag_time() * u_wall) and np.allclose(corr.lag_t_wall(), corr.lag_time() * u_wall ** 2 / nu)
    assert corr.pooled().count.tolist() == [6.0] * n + [4.0] * n
    _, tau_off, state_off, _, _, _ = _tcf_run(False)
    assert torch.equal(state[0], state_off[0]) and torch.equal(state[1], state_off[1])
    assert np.array_equal(tau, tau_off)


def test_every_second_sim_step_halves_the_samples():
    corr, _, _, n, dt, _ = _tcf_run(True, every=2)
    samples = (STEPS * n) // 2
    assert corr.samples == samples
    # stride n, lags 2 n and 8 slots at the most: the schedule is the same, counted in samples
    bases = range(0, samples, n)
    assert corr.count.tolist() == [float(sum(1 for s0 in bases if s0 + lag < samples)) for lag in range(2 * n)]
    live = corr.count > 0
    want = 2 * dt * np.arange(2 * n)
    assert np.abs(corr.lag_time()[:, live] - want[None, live]).max() <= 1e-12 * want[-1]


def test_correlations_are_off_by_default_and_need_a_reset():
    env = fluidgym_amd.make("TCFSmall3D-both-easy-v0", **TCF)
    assert env._hook("flow_timecorr") is None
    with pytest.raises(RuntimeError, match="reset"):
        env.start_flow_time_correlation(4)
    with pytest.raises(RuntimeError, match="no time correlations"):
        env.stop_flow_time_correlation()
    env.reset(seed=4)
    with pytest.raises(ValueError, match="every must be at least 1"):
        env.start_flow_time_correlation(4, every=0)
    with pytest.raises(ValueError, match="channels must be"):
        env.start_flow_time_correlation(4, channels=("u", "v", "p"))          # a 2-D set on a 3-D domain
    with pytest.raises(ValueError, match="more than the 8"):
        env.start_flow_time_correlation(9, stride=1)
    assert env._hook("flow_timecorr") is None
    env.start_flow_time_correlation(3)                                        # the reference's single base
    env.step(torch.zeros(env._zero_action.shape, device=env.cuda_device))
    corr = env.stop_flow_time_correlation()
    assert env._hook("flow_timecorr") is None and corr.full and corr.count.tolist() == [1.0] * 3 and corr.samples == env._n_sim_steps
    assert np.abs(corr.normalized("u")[..., 0] - 1.0).max() == 0.0
    env.close()


def test_rbc2d_records_the_velocity_by_default_and_every_channel_on_request(tmp_path):
    env = fluidgym_amd.make("RBC2D-easy-v0", num_envs=2, n_heaters=4, resolution=8, randomize_initial_state=False, step_length=0.5)
    env.reset(seed=1)
    n = env._n_sim_steps
    env.start_flow_time_correlation(lags=min(n, 4))
    env.step(torch.zeros(2, 4, 1, device="cuda"))
    corr = env.stop_flow_time_correlation()
    ny, nx = env._block.velocity.shape[-2:]
    assert corr.channels == ("u", "v") and corr.coefficient("v").shape == (2, ny, min(n, 4))
    corr.save(tmp_path)
    with np.load(tmp_path / "online_stats_vel_temporal.npz") as z:
        assert z["base_fluctuations"].shape == (2, 2, 1, ny, nx) and z["steps_coefficients"].shape == (min(n, 4), 2, 2, ny)
    env.start_flow_time_correlation(lags=4, stride=2, channels=("u", "v", "p", "T"))
    env.step(torch.zeros(2, 4, 1, device="cuda"))
    corr = env.stop_flow_time_correlation()
    assert corr.channels == ("u", "v", "p", "T") and corr.samples == n
    for c in corr.channels:
        coef = corr.coefficient(c)[..., corr.count > 0]
        ok = ~np.isnan(coef)                                                  # a row without fluctuation (a uniform wall row) is 0 / 0
        assert np.abs(coef[ok]).max() <= 1.0 + 1e-6
    T = corr.coefficient("T")
    print("temperature coefficient at lag 1, env 0:", T[0, :, 1])
    assert np.abs(T[..., 0][~np.isnan(T[..., 0])] - 1.0).max() <= 1e-6
    env.close()
