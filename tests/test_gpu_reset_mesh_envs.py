"""``reset_mesh_envs`` / ``record_mesh_state_bank`` / ``set_mesh_state_bank`` of the cylinder and airfoil envs on the GPU (DESIGN.md
section 6r): one env of a batch restarts from the mesh state bank and the others keep their bits, replay through ``get_state`` /
``set_state``, a recorded bank, independent episodes, the span symmetries and the tracers of the 3-D env, and the refusals."""
import copy

import numpy as np
import pytest
import torch

import fluidgym_amd
from fluidgym_amd.simulation.mb_state_bank import MeshStateBank
from fluidgym_amd.simulation.state_bank import draw_reset_plan
from tests.mb_env_restore_ref import restore_ref
from tests.test_gpu_cylinder import KW, KW3
from tests.test_gpu_mb_tracers import _airfoil

pytestmark = pytest.mark.gpu

FIELDS = ("velocity", "pressure", "boundary_velocity")


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same_up_to_the_sign_of_zero(a, b):
    """Boundary rows after the zero action: the jets are ``profile * 0``, a zero of either sign where the stored state holds ``+0``."""
    a, b = np.asarray(a), np.asarray(b)
    return np.array_equal(a, b) and np.array_equal(_bits(a)[b != 0], _bits(b)[b != 0])


def _fields(env):
    return {k: getattr(env._domain, k).detach().cpu().numpy().copy() for k in FIELDS}


def _cylinder(num_envs=3, **kw):
    return fluidgym_amd.make("CylinderJet2D-easy-v0", num_envs=num_envs, **{**KW, **kw})


def _actions(env, scale=1.0):
    return scale * torch.linspace(-0.8, 0.6, env.num_envs, device=env.cuda_device).reshape(env._zero_action.shape)


def test_one_env_restarts_and_the_others_keep_their_bits():
    env = _cylinder()
    with pytest.raises(RuntimeError):
        env.reset_mesh_envs([1])
    obs0, _ = env.reset(seed=1)
    for _ in range(2):
        env.step(_actions(env))
    before, control = _fields(env), env._last_control.clone()
    assert env.mesh_state_bank is None
    obs = env.reset_mesh_envs([1], randomize=False)
    after = _fields(env)
    assert set(obs) == set(obs0) and all(obs[k].shape == obs0[k].shape and obs[k].shape[0] == 3 for k in obs)
    for k in FIELDS:
        for e in (0, 2):
            assert np.array_equal(_bits(after[k][e]), _bits(before[k][e])), (k, e)
        # env 1: env 0 of the developed state; its jets were at rest there, which is the zero action
        same = _same_up_to_the_sign_of_zero if k == "boundary_velocity" else (lambda a, b: np.array_equal(_bits(a), _bits(b)))
        assert same(after[k][1], env._developed[k][0].cpu().numpy()), k
        assert not np.array_equal(after[k][1], before[k][1]), k
    assert env.mesh_state_bank.size == 1
    assert torch.equal(env._last_control[1], torch.zeros_like(control[1]))
    assert np.array_equal(_bits(env._last_control[[0, 2]]), _bits(control[[0, 2]])) and float(control[0].abs().max()) > 0
    assert env.episode_steps.tolist() == [2, 0, 2] and env.mesh_reset_count.tolist() == [0, 1, 0]
    assert env.reset_mesh_envs(np.array([True, False, True]))["velocity"].shape[0] == 3       # a bool mask
    assert env.episode_steps.tolist() == [0, 0, 0] and env.mesh_reset_count.tolist() == [1, 1, 1]
    env.step(_actions(env))
    assert all(np.isfinite(v).all() for v in _fields(env).values())
    with pytest.raises(NotImplementedError, match="multi-block"):
        env.reset_envs([0])
    with pytest.raises(NotImplementedError, match="reset_mesh_envs"):
        env.reset_envs([0])
    env.reset(seed=1)
    assert env.mesh_reset_count.tolist() == [0, 0, 0]


def test_replay_through_get_state_and_set_state():
    env = _cylinder()
    env.reset(seed=2)
    env.step(_actions(env))
    s = env.get_state()
    rng_before = copy.deepcopy(env._np_rng)

    def run():
        obs = env.reset_mesh_envs([0, 2], randomize=True)
        noisy = _fields(env)
        o, r, *_ = env.step(_actions(env, 0.5))
        return obs, noisy, o, r, _fields(env)

    a = run()
    assert env._np_rng.bit_generator.state == rng_before.bit_generator.state      # a bank of one in 2-D: nothing is drawn
    assert env._last_reset_noise[1:3] == (0.025, 0.025) and env._last_reset_noise[3] == [0, 0]
    env.set_state(s)
    assert env.mesh_reset_count.tolist() == [0, 0, 0]
    b = run()
    for k in a[0]:
        assert torch.equal(a[0][k], b[0][k]) and torch.equal(a[2][k], b[2][k]), k
    assert torch.equal(a[3], b[3])
    for k in FIELDS:
        assert np.array_equal(_bits(a[1][k]), _bits(b[1][k])) and np.array_equal(_bits(a[4][k]), _bits(b[4][k])), k
    # the noise is there, on the chosen envs, and not on the boundary values
    dev = env._developed
    assert not np.array_equal(a[1]["velocity"][0], dev["velocity"][0].cpu().numpy())
    assert _same_up_to_the_sign_of_zero(a[1]["boundary_velocity"][0], dev["boundary_velocity"][0].cpu().numpy())
    assert 0.015 < float(np.std(a[1]["velocity"][0] - dev["velocity"][0].cpu().numpy())) < 0.035
    # env 0 and env 2 draw from streams of their own; a further reset of env 0 moves its counter: another field
    assert not np.array_equal(a[1]["velocity"][0], a[1]["velocity"][2])
    env.reset_mesh_envs([0], randomize=True)
    assert env.mesh_reset_count.tolist() == [2, 0, 1] and env._last_reset_noise[3] == [1]
    assert not np.array_equal(_fields(env)["velocity"][0], a[1]["velocity"][0])
    # a state without the counter loads zeros
    assert set(s) == {"domain", "n_steps", "extra"} and s["extra"]["mesh_reset_count"].tolist() == [0, 0, 0]
    env.set_state({**s, "extra": {k: v for k, v in s["extra"].items() if k != "mesh_reset_count"}})
    assert env.mesh_reset_count.tolist() == [0, 0, 0]


def test_recorded_bank_and_the_sources_drawn_from_it():
    env = _cylinder()
    env.reset(seed=3)
    env.step(_actions(env))
    before, control = _fields(env), env._last_control.clone()
    counters = (env._n_steps, env.episode_steps.copy(), env._sim.total_step)
    bank = env.record_mesh_state_bank(3, every=1)
    assert isinstance(bank, MeshStateBank) and bank.size == 3 and env.mesh_state_bank is bank
    after = _fields(env)
    for k in FIELDS:
        assert np.array_equal(_bits(after[k]), _bits(before[k])), k
    assert (env._n_steps, env._sim.total_step) == (counters[0], counters[2]) and np.array_equal(env.episode_steps, counters[1])
    assert np.array_equal(_bits(env._last_control), _bits(control))
    v = bank.fields["velocity"]
    assert not torch.equal(v[0], v[1]) and not torch.equal(v[1], v[2]) and not torch.equal(v[0], v[2])
    # the default interval: the warm-up span of _randomize_domain spread over the states, in sim steps
    period = 1.0 / 0.3
    assert env._mesh_reset_warmup_env_steps() == 2 * int(period / KW["step_length"]) - 1
    twin = copy.deepcopy(env._np_rng)
    env.reset_mesh_envs([0, 1, 2], randomize=True)
    expected = draw_reset_plan(twin, [0, 1, 2], 3, (), 1, 1, True)
    assert env._last_reset_plan == expected and env._np_rng.bit_generator.state == twin.bit_generator.state
    assert len(set(expected["src"])) > 0
    env.step(_actions(env))
    assert all(np.isfinite(x).all() for x in _fields(env).values())
    env.set_mesh_state_bank(None)                       # back to the bank built on demand
    env.reset_mesh_envs([1], randomize=False)
    assert env.mesh_state_bank.size == 1
    env.set_mesh_state_bank([env.get_state()], env=2)
    assert env.mesh_state_bank.size == 1 and torch.equal(env.mesh_state_bank.fields["pressure"][0], env._domain.pressure[2])


def test_independent_episodes_end_and_restart_per_env():
    env = _cylinder(independent_episodes=True, episode_length=2)
    env.reset(seed=4)
    act = _actions(env)
    *_, truncated, _ = env.step(act)
    assert isinstance(truncated, np.ndarray) and truncated.shape == (3,) and not truncated.any()
    *_, truncated, _ = env.step(act)
    assert truncated.tolist() == [True, True, True]
    with pytest.raises(RuntimeError, match=r"\[0, 1, 2\]"):
        env.step(act)
    env.reset_mesh_envs([1])
    with pytest.raises(RuntimeError, match=r"\[0, 2\]"):
        env.step(act)
    env.reset_mesh_envs([0, 2])
    *_, truncated, _ = env.step(act)
    assert truncated.tolist() == [False, False, False] and env.episode_steps.tolist() == [1, 1, 1]


def test_span_symmetries_noise_stream_and_tracers_of_the_3d_env():
    env = fluidgym_amd.make("CylinderJet3D-easy-v0", num_envs=2, **KW3)
    env.reset(seed=5)
    dom = env._domain
    nz = dom.span_nz()
    assert nz == KW3["resolution"]
    cloud = env.start_mesh_tracers(16, seed=0)
    env.step(torch.full_like(env._zero_action, 0.3))
    assert float(cloud.age[0].max()) > 0 and float(cloud.age[1].max()) > 0
    moved = cloud.positions.clone()
    before = _fields(env)
    twin = copy.deepcopy(env._np_rng)
    env.reset_mesh_envs([0], randomize=True)
    plan = env._last_reset_plan
    assert plan == draw_reset_plan(twin, [0], 1, ("flip_z", "shift_z"), 1, nz, True)      # a mirror, then a roll
    assert env._np_rng.bit_generator.state == twin.bit_generator.state
    assert plan["flip_z"][0] in (0, 1) and 0 <= plan["shift_z"][0] < nz and plan["flip_x"] == [0] and plan["shift_x"] == [0]
    bank = {k: t.cpu().numpy() for k, t in env.mesh_state_bank.fields.items()}
    records = [(0, plan["src"][0], plan["flip_z"][0], plan["shift_z"][0])]
    seed, sv, sp, episodes = env._last_reset_noise
    assert (seed, sv, sp, episodes) == (5, 0.025, 0.025, [0])
    ev, ep, eb = restore_ref(dom.blocks, 3, nz, before["velocity"], before["pressure"], before["boundary_velocity"], bank["velocity"],
                             bank["pressure"], bank["boundary_velocity"], records, (seed, sv, sp, episodes))
    after = _fields(env)
    assert np.array_equal(_bits(after["velocity"]), _bits(ev)) and np.array_equal(_bits(after["pressure"]), _bits(ep))
    assert _same_up_to_the_sign_of_zero(after["boundary_velocity"], eb)       # the jets of the stored state were at rest: the zero action
    # the tracers of the chosen env return to their seeds, those of the other env stay
    assert torch.equal(cloud.positions[0], cloud.seed_positions[0]) and float(cloud.age[0].abs().max()) == 0
    assert torch.equal(cloud.positions[1], moved[1]) and float(cloud.age[1].max()) > 0
    env.step(torch.full_like(env._zero_action, 0.3))
    assert all(np.isfinite(x).all() for x in _fields(env).values())


def test_airfoil_takes_its_own_amplitude():
    env = _airfoil()
    env.reset(seed=6)
    act = torch.zeros_like(env._zero_action)
    env.step(act)
    before = _fields(env)
    env.reset_mesh_envs([0], randomize=True)
    assert env._last_reset_noise[1:3] == (0.01, 0.01)
    after = _fields(env)
    assert np.array_equal(_bits(after["velocity"][1]), _bits(before["velocity"][1]))
    delta = after["velocity"][0] - env._developed["velocity"][0].cpu().numpy()
    assert 0.006 < float(np.std(delta)) < 0.014
    obs, reward, *_ = env.step(act)
    assert all(bool(torch.isfinite(v).all()) for v in obs.values()) and bool(torch.isfinite(reward).all())
    assert all(np.isfinite(x).all() for x in _fields(env).values())
    assert env._mesh_reset_warmup_env_steps() == int(0.05 * 3)


def test_refusals():
    per_env = fluidgym_amd.make("CylinderJet2D-easy-v0", num_envs=2, **{**KW, "reynolds_number": [100.0, 150.0]})
    per_env.reset(seed=7)
    with pytest.raises(NotImplementedError, match="one parameter value per env"):
        per_env.reset_mesh_envs([0])
    rbc = fluidgym_amd.make("RBC2D-easy-v0", num_envs=2, n_heaters=4, resolution=8, step_length=0.1, load_initial_domain=False,
                            load_domain_statistics=False, randomize_initial_state=False)
    rbc.reset(seed=7)
    for call in (lambda: rbc.reset_mesh_envs([0]), lambda: rbc.set_mesh_state_bank([]), lambda: rbc.record_mesh_state_bank(2)):
        with pytest.raises(NotImplementedError, match="reset_envs"):
            call()
