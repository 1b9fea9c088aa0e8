"""``fluidgym_amd.wrappers`` on the GPU, on the small envs of the suite: the noisy observations and actions are the clean ones of an
identically seeded bare twin plus the NumPy checker's noise (``tests/obs_noise_ref.py``), bit for bit; ``reset_envs`` leaves the streams
of the untouched envs in place; ``get_state`` / ``set_state`` replay the noise."""
import numpy as np
import pytest
import torch

import fluidgym_amd
from fluidgym_amd.wrappers import ActionNoise, FlattenObservation, FluidWrapper, ObsExtraction, SensorNoise
from tests import obs_noise_ref as R

pytestmark = pytest.mark.gpu

SMALL = dict(step_length=0.1, load_initial_domain=False, load_domain_statistics=False)
CASES = {
    "rbc2d-batch": ("RBC2D-easy-v0", dict(num_envs=3, n_heaters=4, resolution=8, **SMALL)),
    # (a window of one heater: the default of 11 does not fit two heaters)
    "rbc3d-marl-batch": ("RBC3D-easy-v0", dict(num_envs=2, n_heaters=2, resolution=4, use_marl=True, local_obs_window=1, **SMALL)),
    "rbc2d-f64-unbatched": ("RBC2D-easy-v0", dict(dtype=torch.float64, n_heaters=4, resolution=8, **SMALL)),
}
SIGMA, NOISE_SEED, ENV_SEED = 0.05, 0x5EED0000BEEF, 11


@pytest.fixture(scope="module")
def twins():
    """Two bare envs per case, made once; every test resets them with the same seed and wraps them anew (fresh counters)."""
    made = {}

    def get(case):
        if case not in made:
            env_id, kw = CASES[case]
            made[case] = (fluidgym_amd.make(env_id, **kw), fluidgym_amd.make(env_id, **kw))
        return made[case]

    yield get
    for pair in made.values():
        for env in pair:
            env.close()


class Tap(FluidWrapper):
    """Keeps the very tensors the env handed out, to see afterwards that nobody wrote them."""

    def reset(self, seed=None, randomize=None):
        self.last, info = self._env.reset(seed=seed, randomize=randomize)
        return self.last, info

    def step(self, action):
        self.last, *rest = self._env.step(action)
        return (self.last, *rest)


def _rows(t, space):
    lead = t.dim() - len(space.shape)
    return int(np.prod(t.shape[:lead], dtype=np.int64)) if lead else 1


def _checker(tensors, tags, rows, counters, first_row=0, sigma=SIGMA):
    """The checker's ``t + sigma z`` for device tensors of ``rows`` rows each, as host arrays of the tensors' shapes."""
    dtype = {torch.float32: 0, torch.float64: 1}[tensors[0].dtype]
    segs = [dict(src=t.detach().cpu().numpy().reshape(rows, -1), tag=tag, sigma=sigma) for t, tag in zip(tensors, tags)]
    ids = None if first_row == 0 else [first_row + r for r in range(rows)]
    out = R.noise_add(segs, rows, counters, ids, NOISE_SEED, dtype)
    return [o.reshape(tuple(t.shape)) for o, t in zip(out, tensors)]


def _same_bits(t: torch.Tensor, want: np.ndarray) -> bool:
    got = t.detach().cpu().numpy()
    bits = np.uint32 if got.dtype == np.float32 else np.uint64
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got.view(bits), want.view(bits))


def _assert_noisy(noisy, clean, space, counters, first_row=0):
    keys = sorted(clean)
    rows = _rows(clean[keys[0]], space.spaces[keys[0]])
    want = _checker([clean[k] for k in keys], range(len(keys)), rows, counters(rows), first_row)
    assert list(noisy) == list(clean)
    for k, w in zip(keys, want):
        assert _same_bits(noisy[k], w), f"{k}: not clean + sigma z of the checker"
        assert not torch.equal(noisy[k], clean[k])


def _action(env, scale):
    z = env.unwrapped._zero_action if isinstance(env, FluidWrapper) else env._zero_action
    return scale * torch.linspace(-1.0, 1.0, z.numel(), device=z.device, dtype=z.dtype).reshape(z.shape)


@pytest.mark.parametrize("case, first_row", [("rbc2d-batch", 0), ("rbc3d-marl-batch", 7), ("rbc2d-f64-unbatched", 0)])
def test_sensor_noise_is_the_twin_plus_the_checker(twins, case, first_row):
    bare, inner = twins(case)
    tap = Tap(inner)
    env = SensorNoise(tap, SIGMA, NOISE_SEED, first_row=first_row)
    clean, _ = bare.reset(seed=ENV_SEED)
    noisy, _ = env.reset(seed=ENV_SEED)
    space = bare.observation_space
    _assert_noisy(noisy, clean, space, lambda rows: [[1, 0]] * rows, first_row)
    for step in (1, 2):
        a = _action(bare, 0.3 * step)
        clean, reward, *_ = bare.step(a)
        noisy, reward_w, *_ = env.step(a.clone())
        _assert_noisy(noisy, clean, space, lambda rows: [[1, step]] * rows, first_row)
        assert torch.equal(reward, reward_w)
        for k in clean:      # the env's own tensors were not written
            assert torch.equal(tap.last[k], clean[k]) and tap.last[k].data_ptr() != noisy[k].data_ptr()
    # a second episode draws other numbers
    clean, _ = bare.reset(seed=ENV_SEED)
    noisy, _ = env.reset(seed=ENV_SEED)
    _assert_noisy(noisy, clean, space, lambda rows: [[2, 0]] * rows, first_row)


@pytest.mark.parametrize("case", list(CASES))
def test_action_noise_is_the_twin_stepped_with_the_checkers_action(twins, case):
    bare, inner = twins(case)
    env = ActionNoise(inner, SIGMA, NOISE_SEED)
    o0, _ = bare.reset(seed=ENV_SEED)
    o0w, _ = env.reset(seed=ENV_SEED)
    assert all(torch.equal(o0[k], o0w[k]) for k in o0)
    rows = _rows(bare._zero_action, bare.action_space)
    for step in (1, 2):
        a = _action(bare, 0.2 * step)
        noisy_a = _checker([a], [128], rows, [[1, step]] * rows)[0]
        assert not np.array_equal(noisy_a, a.cpu().numpy())
        obs, reward, *_ = bare.step(torch.from_numpy(noisy_a).to(a.device))
        obs_w, reward_w, *_ = env.step(a)
        assert torch.equal(reward, reward_w)
        for k in obs:
            assert torch.equal(obs[k], obs_w[k]), k
    assert env.noise_counters.cpu().tolist() == [[1, 2]] * rows


@pytest.mark.parametrize("case", ["rbc2d-batch", "rbc3d-marl-batch"])
def test_reset_envs_keeps_the_streams_of_the_other_envs(twins, case):
    bare, inner = twins(case)
    env = SensorNoise(inner, SIGMA, NOISE_SEED)
    bare.reset(seed=ENV_SEED)
    env.reset(seed=ENV_SEED)
    a = _action(bare, 0.25)
    bare.step(a)
    before, *_ = env.step(a)
    clean = bare.reset_envs([1])
    after = env.reset_envs([1])
    B = bare.num_envs
    others = [e for e in range(B) if e != 1]
    for k in before:
        assert torch.equal(after[k][others], before[k][others]), f"{k}: an unchosen env's noisy observation changed"
        assert not torch.equal(after[k][1], before[k][1])
    per_env = _rows(clean["temperature"], bare.observation_space.spaces["temperature"]) // B
    words = [[2, 0] if r // per_env == 1 else [1, 1] for r in range(B * per_env)]
    assert env.noise_counters.cpu().tolist() == words
    _assert_noisy(after, clean, bare.observation_space, lambda rows: words)
    # a bool mask names the same envs
    clean = bare.reset_envs([False, True] + [False] * (B - 2))
    after = env.reset_envs(torch.tensor([False, True] + [False] * (B - 2)))
    words = [[3, 0] if r // per_env == 1 else [1, 1] for r in range(B * per_env)]
    _assert_noisy(after, clean, bare.observation_space, lambda rows: words)


@pytest.mark.parametrize("case", list(CASES))
def test_state_round_trip_replays_the_noise(twins, case):
    """FlattenObservation(SensorNoise(ObsExtraction(ActionNoise(env)))): get_state, two steps, set_state, the same two steps."""
    _, inner = twins(case)
    keys = ["velocity", "temperature"]
    env = FlattenObservation(SensorNoise(ObsExtraction(ActionNoise(inner, SIGMA, NOISE_SEED + 1), keys), SIGMA, NOISE_SEED))
    env.reset(seed=ENV_SEED)
    actions = [_action(env, 0.1), _action(env, -0.2), _action(env, 0.3)]
    env.step(actions[0])
    state = env.get_state()
    assert {"sensor_noise_counters", "action_noise_counters", "domain"} <= set(state)
    first = [env.step(a) for a in actions[1:]]
    assert not torch.equal(first[0][0], first[1][0])
    env.set_state(state)
    again = [env.step(a) for a in actions[1:]]
    sub = inner.observation_space.spaces
    for (flat, reward, _, _, info), (flat2, reward2, _, _, info2) in zip(first, again):
        assert torch.equal(flat, flat2) and torch.equal(reward, reward2)
        assert set(info) >= {"original_velocity", "original_temperature"} and "original_pressure" not in info
        assert torch.equal(info["original_velocity"], info2["original_velocity"])
        # the flat observation is the flattening of the noisy dict: temperature, then velocity, after the leading axes
        lead = tuple(info["original_temperature"].shape[: info["original_temperature"].dim() - len(sub["temperature"].shape)])
        want = torch.cat([info["original_temperature"].reshape(lead + (-1,)), info["original_velocity"].reshape(lead + (-1,))], dim=-1)
        assert torch.equal(flat, want) and flat.shape == lead + env.observation_space.shape


def test_wrappers_on_a_parallel_env():
    """``ParallelFluidEnv`` (one rank, no collectives): observations stacked over the envs, one info dict per env.  The noisy flat
    observation is the flattening of the twin's clean dict plus the checker's noise, and every env's info keeps its own originals."""
    from fluidgym_amd.envs import ParallelFluidEnv

    env_id, kw = CASES["rbc2d-batch"]
    kw = dict(kw, num_envs=2)
    bare, inner = ParallelFluidEnv(env_id, **kw), ParallelFluidEnv(env_id, **kw)
    try:
        env = FlattenObservation(SensorNoise(inner, SIGMA, NOISE_SEED))
        assert env.unwrapped is inner and env.num_envs == 2
        clean, _ = bare.reset(seed=ENV_SEED)
        flat, infos = env.reset(seed=ENV_SEED)
        a = _action(bare.local_env, 0.3)
        clean, reward, *_ = bare.step(a)
        flat, reward_w, _, _, infos = env.step(a)
        assert torch.equal(reward, reward_w) and len(infos) == 2
        keys = sorted(clean)
        noisy = dict(zip(keys, _checker([clean[k] for k in keys], range(len(keys)), 2, [[1, 1]] * 2)))
        want = np.concatenate([noisy["temperature"].reshape(2, -1), noisy["velocity"].reshape(2, -1)], axis=1)
        assert _same_bits(flat, want)
        for e in range(2):
            assert _same_bits(infos[e]["original_pressure"], noisy["pressure"][e])
    finally:
        bare.close()
        inner.close()
