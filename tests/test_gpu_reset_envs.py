"""``FluidEnv.reset_envs`` / ``reset(per_env=True)`` / ``independent_episodes`` on the GPU: RBC2D-easy-v0 (four heaters: 32 cells along x) with three envs and short
env steps, the channel env (no symmetry, an action filter per env), and the refusals."""
import numpy as np
import pytest
import torch

import fluidgym_amd
from fluidgym_amd.envs import ParallelFluidEnv

pytestmark = pytest.mark.gpu

RBC = dict(num_envs=3, n_heaters=4, resolution=8, step_length=0.1, load_initial_domain=False, load_domain_statistics=False)      # two sim steps per env step


def _rbc(**kw):
    return fluidgym_amd.make("RBC2D-easy-v0", **{**RBC, **kw})


def _state(env):
    blk = env._domain.getBlock(0)
    out = {"u": blk.velocity, "p": blk.pressure, "T": blk.passiveScalar}
    out.update({f"bs{f}": t for f, t in env._domain.solver.bscal.items()})
    out.update({f"bv{f}": t for f, t in env._domain.solver.bvel.items()})
    return {k: v.detach().cpu().numpy().copy() for k, v in out.items()}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_reset_envs_restores_one_env_and_leaves_the_others():
    env = _rbc(randomize_initial_state=False)
    obs0, _ = env.reset(seed=3)
    assert env.episode_steps.dtype == np.int64 and env.episode_steps.tolist() == [0, 0, 0]
    act = torch.zeros(env._zero_action.shape, device=env.cuda_device)
    act[:, 0] = 1.0
    for _ in range(2):
        env.step(act)
    assert env.episode_steps.tolist() == [2, 2, 2]
    before = _state(env)
    obs = env.reset_envs([1])
    after = _state(env)
    assert set(obs) == set(obs0) and all(obs[k].shape == obs0[k].shape and obs[k].shape[0] == 3 for k in obs)
    for k in before:
        for e in (0, 2):
            assert np.array_equal(_bits(after[k][e]), _bits(before[k][e])), (k, e)
    assert not np.array_equal(after["T"][1], before["T"][1])
    # without randomize and with a bank of one: env 1 is env 0 of the generated initial state, under the zero action
    bank = env.state_bank
    assert bank is not None and bank.size == 1
    assert np.array_equal(_bits(after["u"][1]), _bits(bank.fields["velocity"][0].cpu().numpy()))
    assert np.array_equal(_bits(after["T"][1]), _bits(bank.fields["scalar"][0].cpu().numpy()))
    assert env.episode_steps.tolist() == [2, 0, 2]
    assert env.reset_envs(np.array([True, False, True]))["temperature"].shape[0] == 3      # a bool mask
    assert env.episode_steps.tolist() == [0, 0, 0]
    env.step(act)
    assert env.episode_steps.tolist() == [1, 1, 1]
    assert all(np.isfinite(v).all() for v in _state(env).values())
    with pytest.raises(ValueError):
        env.reset_envs([3])
    with pytest.raises(ValueError):
        env.reset_envs([1, 1])
    env.close()


def test_explicit_state_bank_and_randomised_reset_of_chosen_envs():
    env = _rbc(randomize_initial_state=False)
    env.reset(seed=4)
    zero = torch.zeros(env._zero_action.shape, device=env.cuda_device)
    states = []
    for _ in range(2):
        env.step(zero)
        states.append(env.get_state())
    env.set_state_bank(states)                   # every env of both snapshots: six entries
    assert env.state_bank.size == 6
    before = _state(env)
    rng = np.random.default_rng(4)
    rng.bit_generator.state = env._np_rng.bit_generator.state
    env.reset_envs([2, 0], randomize=True)
    plan = env._last_reset_plan
    want = [(int(rng.integers(0, 6)), int(rng.uniform(0.0, 1.0) > 0.5), int(rng.integers(0, env._x))) for _ in range(2)]
    assert plan["env"] == [0, 2] and list(zip(plan["src"], plan["flip_x"], plan["shift_x"])) == want
    assert plan["flip_z"] == [0, 0] and plan["shift_z"] == [0, 0]
    after = _state(env)
    for k in before:
        assert np.array_equal(_bits(after[k][1]), _bits(before[k][1])), k
    # the chosen envs: the stored state under the symmetry, plus noise of the family's amplitude (0.05), clamped temperature
    bank_u = env.state_bank.fields["velocity"].cpu().numpy()
    for e, (src, fx, sx) in zip(plan["env"], want):
        ref = bank_u[src]
        if fx:
            ref = ref[..., ::-1] * np.array([-1.0, 1.0], np.float32).reshape(2, 1, 1)
        ref = np.roll(ref, sx, axis=-1)
        noise = after["u"][e] - ref
        assert 0.03 < noise.std() < 0.07 and np.abs(noise).max() < 0.05 * 6
    assert after["T"].min() >= env._T_cold and after["T"].max() <= env._T_hot + env._heater_limit
    env.step(zero)
    assert all(np.isfinite(v).all() for v in _state(env).values())
    env.close()


def test_reset_per_env_gives_every_env_its_own_symmetry_and_repeats():
    """Seed 12 draws (after the normal reset's three numbers) mirror / roll (0, 30), (0, 15), (1, 7) for the three envs.  The bank holds
    one state whose temperature is a wave along x, so a rolled or mirrored image differs from it by far more than the noise."""
    runs = []
    for _ in range(2):
        env = _rbc(randomize_initial_state=True)
        env.reset(seed=1, randomize=False)
        st = env.get_state()
        nx = env._x
        wave = 0.5 + 0.4 * torch.sin(2 * np.pi * torch.arange(nx, device=env.cuda_device) / nx + 0.3)
        st["domain"]["scalar"].copy_(wave.expand_as(st["domain"]["scalar"]))
        env.set_state_bank([st], env=0)
        obs, info = env.reset(seed=12, randomize=True, per_env=True)
        runs.append((_state(env), dict(env._last_reset_plan), {k: v.cpu().numpy() for k, v in obs.items()}, wave.cpu().numpy()))
        assert info == {} and env.episode_steps.tolist() == [0, 0, 0]
        env.close()
    (s0, plan, o0, wave), (s1, plan1, o1, _) = runs
    assert plan == plan1 and plan["env"] == [0, 1, 2] and plan["src"] == [0, 0, 0]
    assert plan["flip_x"] == [0, 0, 1] and plan["shift_x"] == [30, 15, 7]          # the rolls differ
    for k in s0:
        assert np.array_equal(_bits(s0[k]), _bits(s1[k])), k                      # reproducible for the same seed
    for k in o0:
        assert np.array_equal(o0[k], o1[k]), k
    T = s0["T"][:, 0]                                                             # [B, y, x]
    for e in range(3):
        ref = np.roll(wave[::-1] if plan["flip_x"][e] else wave, plan["shift_x"][e])
        assert np.abs(T[e] - ref[None, :]).max() < 6 * 0.05, e                    # each env: its own image of the state, plus noise
    for a, b in ((0, 1), (0, 2), (1, 2)):
        assert np.abs(T[a] - T[b]).max() > 0.4, (a, b)                            # and the envs differ by more than noise


def test_default_reset_draws_what_it_drew_before():
    """reset(seed) without per_env: the parent's draws -- mirror, roll, warm-up time (rbc.py:_randomize_domain; no initial-domain
    index without files on disk) -- and nothing else: the generator's next number is the fourth of its stream."""
    env = _rbc(randomize_initial_state=True)
    env.reset(seed=11)
    rng = np.random.default_rng(11)
    rng.uniform(0.0, 1.0), rng.integers(0, env._x), rng.uniform(1.0, 2.0)
    fourth = int(rng.integers(0, 2 ** 31))
    assert fourth == 1072191045
    assert int(env._np_rng.integers(0, 2 ** 31)) == fourth
    assert env.state_bank is None
    env.close()


def test_independent_episodes_truncate_per_env():
    act = None
    for independent in (False, True):
        env = _rbc(randomize_initial_state=False, episode_length=2, independent_episodes=independent)
        env.reset(seed=5)
        act = torch.zeros(env._zero_action.shape, device=env.cuda_device)
        truncated = env.step(act)[3]
        if not independent:
            assert truncated is False                       # what it returns today: one bool for the batch
            assert env.step(act)[3] is True
            with pytest.raises(RuntimeError, match=r"Episode has already terminated\. Call 'reset\(\)' first\."):
                env.step(act)
        else:
            assert isinstance(truncated, np.ndarray) and truncated.dtype == np.bool_ and truncated.tolist() == [False] * 3
            env.reset_envs([1], randomize=False)
            assert env.step(act)[3].tolist() == [True, False, True]
            with pytest.raises(RuntimeError, match=r"Episode has already terminated in envs \[0, 2\]"):
                env.step(act)
            env.reset_envs([0, 2], randomize=False)
            assert env.step(act)[3].tolist() == [False, True, False]
        env.close()


def test_channel_env_resets_one_env_without_a_symmetry():
    env = fluidgym_amd.make("ChannelJet2D-v0", num_envs=2, resolution_x=64, resolution_y=32, randomize_initial_state=False,
                            load_initial_domain=False, load_domain_statistics=False)
    env.reset(seed=2)
    assert env._reset_symmetries() == ()
    act = torch.full(env._zero_action.shape, 0.5, device=env.cuda_device)
    for _ in range(2):
        env.step(act)
    blk = env._domain.getBlock(0)
    u_before = blk.velocity.cpu().numpy().copy()
    out_before = env._domain.solver.bvel[1].cpu().numpy().copy()
    assert float(env._current_action.abs().min()) > 0
    env.reset_envs([0], randomize=True)
    u_after = blk.velocity.cpu().numpy()
    assert np.array_equal(_bits(u_after[1]), _bits(u_before[1]))
    assert np.array_equal(_bits(env._domain.solver.bvel[1].cpu().numpy()[1]), _bits(out_before[1]))
    noise = u_after[0] - env.state_bank.fields["velocity"][0].cpu().numpy()
    assert 0.03 < noise.std() < 0.07
    assert env._current_action.reshape(-1).tolist()[0] == 0.0 and env._current_action.reshape(-1).tolist()[1] != 0.0
    assert float(env._domain.solver.bvel[2][0].abs().max()) == 0.0 and float(env._domain.solver.bvel[2][1].abs().max()) > 0
    env.step(act)
    assert np.isfinite(blk.velocity.cpu().numpy()).all()
    env.close()


def test_refusals():
    env = _rbc(randomize_initial_state=False)
    with pytest.raises(RuntimeError, match="reset"):
        env.reset_envs([0])
    env.reset(seed=1)
    env.start_flow_time_correlation(lags=4)
    with pytest.raises(RuntimeError, match="time-correlation"):
        env.reset_envs([0])
    env.stop_flow_time_correlation()
    env.start_flow_statistics()                  # the other recorders keep running
    env.reset_envs([0])
    env.stop_flow_statistics()
    env.close()
    het = fluidgym_amd.make("RBC2D-easy-v0", **{**RBC, "rayleigh_number": [8e4, 9e4, 1e5], "randomize_initial_state": False})
    het.reset(seed=1)
    with pytest.raises(NotImplementedError, match="one parameter value per env"):
        het.reset_envs([0])
    het.close()
    cyl = fluidgym_amd.make("CylinderJet2D-easy-v0", num_envs=2, resolution=8, initial_domain_steps=6, randomize_initial_state=False,
                            step_length=0.05, dt=0.01, episode_length=3)       # the smallest cylinder the suite builds
    cyl.reset(seed=1)
    with pytest.raises(NotImplementedError, match="multi-block"):
        cyl.reset_envs([0])
    cyl.close()
    with pytest.raises(NotImplementedError, match="reset_envs is not implemented for ParallelFluidEnv."):
        ParallelFluidEnv.reset_envs(object.__new__(ParallelFluidEnv), [0])
    with pytest.raises(NotImplementedError, match="set_state_bank is not implemented for ParallelFluidEnv."):
        ParallelFluidEnv.set_state_bank(object.__new__(ParallelFluidEnv), [])
