"""``NormalizeObservation`` / ``NormalizeReward`` end to end on the GPU, on the small envs of the suite: the
wrapped observations and rewards are the NumPy checker (``tests/obs_normalize_ref.py``) applied to the raw ones of an identically
seeded bare twin, within the checker's derived bounds; ``reset_envs`` merges the rows of the chosen envs only; ``get_state`` /
``set_state`` replay bit for bit; ``freeze`` leaves the record alone.

The bounds are those of the checker's docstring at the scale of the env's data: records within ``C N 2^-52`` of ``x_max`` and
``x_max^2 N`` (``x_max`` the largest magnitude seen), fp32 outputs within ``2^-23 max(1, |ref|)``, fp64 outputs within the propagated
record error times the slot's own ``rstd`` (an env's slots are not held to a standard deviation of 0.25, so ``rstd`` is not bounded by 4
but by ``1 / sqrt(epsilon)``)."""
import numpy as np
import pytest
import torch

import fluidgym_amd
from fluidgym_amd.wrappers import FlattenObservation, FluidWrapper, NormalizeObservation, NormalizeReward, SensorNoise
from tests import obs_normalize_ref as R

pytestmark = pytest.mark.gpu

SMALL = dict(step_length=0.1, load_initial_domain=False, load_domain_statistics=False)
CASES = {
    "rbc2d-batch": ("RBC2D-easy-v0", dict(num_envs=3, n_heaters=4, resolution=8, **SMALL)),
    "rbc2d-f64-batch": ("RBC2D-easy-v0", dict(num_envs=2, dtype=torch.float64, n_heaters=4, resolution=8, **SMALL)),
    "tcf-marl-batch": ("TCFSmall3D-both-easy-v0", dict(num_envs=2, randomize_initial_state=False, resolution_x_z=16, resolution_y=16,
                                                       step_length=0.6)),
}
ENV_SEED, EPS, GAMMA = 11, 1e-8, 0.9


@pytest.fixture(scope="module")
def twins():
    """Two bare envs per case, made once; every test resets them with the same seed and wraps them anew (fresh records)."""
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


def _action(env, scale):
    z = env.unwrapped._zero_action if isinstance(env, FluidWrapper) else env._zero_action
    return scale * torch.linspace(-1.0, 1.0, z.numel(), device=z.device, dtype=z.dtype).reshape(z.shape)


def _rows(t, space):
    lead = t.dim() - len(space.shape)
    return int(np.prod(t.shape[:lead], dtype=np.int64)) if lead else 1


class Checker:
    """The checker's records of an observation dict (or single tensor), fed with the twin's raw observations."""

    def __init__(self, space, pooled=False, clip=None):
        self.space, self.pooled, self.clip = space, pooled, clip
        self.recs, self.x_max = {}, {}

    def _flat(self, obs):
        if not isinstance(obs, dict):
            return {"": obs.detach().cpu().numpy().reshape(_rows(obs, self.space), -1)}
        return {k: v.detach().cpu().numpy().reshape(_rows(v, self.space.spaces[k]), -1) for k, v in obs.items()}

    def update(self, obs, rows=None):
        for k, x in self._flat(obs).items():
            self.recs.setdefault(k, R.Record(pooled=self.pooled)).update(x, rows=rows)
            self.x_max[k] = max(self.x_max.get(k, 0.0), float(np.max(np.abs(x))))

    def hold(self, got, obs, what):
        """``got`` (the wrapper's output for the raw ``obs``) within the derived bounds of the checker's current records."""
        got = self._flat(got)
        for k, x in self._flat(obs).items():
            rec = self.recs[k]
            want = rec.apply(x, EPS, self.clip)
            y = got[k]
            assert y.dtype == want.dtype and y.shape == want.shape
            if y.dtype == np.float32:
                tol = 2.0 ** -23 * np.maximum(1.0, np.abs(want.astype(np.float64)))
            else:
                t_mean, t_m2 = R.tolerances(rec.n, self.x_max[k])
                rstd = 1.0 / np.sqrt(rec.m2 / rec.n + EPS)
                tol = rstd * t_mean + np.abs(want) * (rstd ** 2 / 2.0) * (t_m2 / rec.n) + 4.0 * 2.0 ** -52 * np.abs(want)
            dev = np.abs(y.astype(np.float64) - want.astype(np.float64))
            print(f"{what} {k}: N {rec.n} worst |y - ref| {float(np.max(dev)):.3e}, smallest bound {float(np.min(tol)):.3e}")
            assert np.all(dev <= tol), (what, k)

    def hold_records(self, wrapper, what):
        stats = wrapper.statistics
        for k, rec in self.recs.items():
            count, mean, var = stats[k or "observation"]
            t_mean, t_m2 = R.tolerances(rec.n, self.x_max[k])
            assert count == rec.n, (what, k, count, rec.n)
            assert np.all(np.abs(mean.cpu().numpy() - rec.mean) <= t_mean), (what, k)
            assert np.all(np.abs(var.cpu().numpy() * count - rec.m2) <= t_m2 + 2.0 ** -52 * np.abs(rec.m2)), (what, k)


def _hold_reward(got, raw, ref, what):
    """The scaled reward against the checker's return record: fp32 within one rounding, the record within its bounds at the scale of G."""
    want = ref.step(raw.detach().cpu().numpy().reshape(-1), EPS)
    y = got.detach().cpu().numpy().reshape(-1)
    assert got.shape == raw.shape and got.dtype == raw.dtype
    g_max = max(float(np.max(np.abs(ref.G))), 1e-30)
    if y.dtype == np.float32:
        tol = 2.0 ** -23 * np.maximum(1.0, np.abs(want.astype(np.float64)))
    else:
        rstd = 1.0 / np.sqrt(ref.rec.m2 / ref.rec.n + EPS)
        tol = np.abs(want) * (rstd ** 2 / 2.0) * (R.tolerances(ref.rec.n, g_max)[1] / ref.rec.n) + 4.0 * 2.0 ** -52 * np.abs(want)
    assert np.all(np.abs(y.astype(np.float64) - want.astype(np.float64)) <= tol), what
    return g_max


def _hold_reward_record(wrapper, ref, g_max, what):
    n, mean, var = wrapper.statistics
    t_mean, t_m2 = R.tolerances(ref.rec.n, g_max)
    assert n == ref.rec.n and abs(float(mean) - ref.rec.mean) <= t_mean and abs(float(var) * n - ref.rec.m2) <= t_m2 + 2.0 ** -52 * ref.rec.m2, what
    assert np.all(np.abs(wrapper.returns.cpu().numpy() - ref.G) <= 4 * 2.0 ** -52 * g_max), what


def test_rbc_batch_against_the_twin_with_reset_envs_state_and_freeze(twins):
    bare, inner = twins("rbc2d-batch")
    tap = Tap(inner)
    obs_w = NormalizeObservation(tap)
    env = NormalizeReward(obs_w, gamma=GAMMA)
    space = bare.observation_space
    chk = Checker(space)
    raw, _ = bare.reset(seed=ENV_SEED)
    got, _ = env.reset(seed=ENV_SEED)
    chk.update(raw)
    chk.hold(got, raw, "reset")
    assert list(got) == list(raw) and all(got[k].shape == raw[k].shape and got[k].dtype == raw[k].dtype for k in raw)
    rows = _rows(raw["temperature"], space.spaces["temperature"])
    per_env = rows // 3
    ret = R.ReturnRecord(3, GAMMA)
    for step in (1, 2):
        a = _action(bare, 0.3 * step)
        raw, reward, *_ = bare.step(a)
        got, reward_w, *_ = env.step(a.clone())
        chk.update(raw)
        chk.hold(got, raw, f"step {step}")
        g_max = _hold_reward(reward_w, reward, ret, f"reward step {step}")
        for k in raw:      # the env's own tensors were not written; the outputs are new tensors
            assert torch.equal(tap.last[k], raw[k]) and tap.last[k].data_ptr() != got[k].data_ptr()
    chk.hold_records(obs_w, "after two steps")
    _hold_reward_record(env, ret, g_max, "after two steps")
    assert obs_w.statistics["temperature"][0] == 3 * rows and env.statistics[0] == 6
    # reset_envs([1]): the rows of env 1 join the record, every row is normalised, only env 1's return is zeroed
    n_before = obs_w.statistics["temperature"][0]
    raw = bare.reset_envs([1])
    got = env.reset_envs([1])
    chk.update(raw, rows=list(range(per_env, 2 * per_env)))
    chk.hold(got, raw, "reset_envs")
    assert obs_w.statistics["temperature"][0] == n_before + per_env
    G = env.returns.cpu().numpy()
    assert G[1] == 0.0 and G[0] != 0.0 and G[2] != 0.0
    ret.G[1] = 0.0
    a = _action(bare, -0.2)
    raw, reward, *_ = bare.step(a)
    got, reward_w, *_ = env.step(a.clone())
    chk.update(raw)
    chk.hold(got, raw, "step after reset_envs")
    g_max = _hold_reward(reward_w, reward, ret, "reward after reset_envs")
    chk.hold_records(obs_w, "at the end")
    _hold_reward_record(env, ret, g_max, "at the end")
    # get_state -> two steps -> set_state -> the same two steps: every output and the records bit for bit
    actions = [_action(env, 0.1), _action(env, -0.3)]
    state = env.get_state()
    assert {"obs_normalizer", "reward_normalizer", "domain"} <= set(state)
    first = [env.step(a) for a in actions]
    rec_first = (obs_w.get_state()["obs_normalizer"], env.get_state()["reward_normalizer"])
    env.set_state(state)
    assert obs_w.statistics["temperature"][0] == n_before + per_env + rows
    again = [env.step(a) for a in actions]
    rec_again = (obs_w.get_state()["obs_normalizer"], env.get_state()["reward_normalizer"])
    for (o1, r1, *_), (o2, r2, *_) in zip(first, again):
        assert torch.equal(r1, r2) and all(torch.equal(o1[k], o2[k]) for k in o1)
    assert rec_first[0]["n"] == rec_again[0]["n"] and rec_first[1]["n"] == rec_again[1]["n"]
    for k in rec_first[0]["mean"]:
        assert torch.equal(rec_first[0]["mean"][k], rec_again[0]["mean"][k]) and torch.equal(rec_first[0]["M2"][k], rec_again[0]["M2"][k])
    assert all(torch.equal(rec_first[1][k], rec_again[1][k]) for k in ("mean", "M2", "G"))
    # freeze(): a step normalises with the record as it is; train() / val() do not touch the switch
    env.freeze(), obs_w.freeze()
    env.val(), env.train()
    assert not env.updating and not obs_w.updating
    kept = (obs_w.get_state()["obs_normalizer"], env.get_state()["reward_normalizer"])
    G_before = env.returns.clone()
    got, reward_w, *_ = env.step(actions[0])
    now = (obs_w.get_state()["obs_normalizer"], env.get_state()["reward_normalizer"])
    assert kept[0]["n"] == now[0]["n"] and kept[1]["n"] == now[1]["n"]
    assert all(torch.equal(kept[0]["mean"][k], now[0]["mean"][k]) and torch.equal(kept[0]["M2"][k], now[0]["M2"][k]) for k in kept[0]["mean"])
    assert torch.equal(kept[1]["mean"], now[1]["mean"]) and torch.equal(kept[1]["M2"], now[1]["M2"])
    assert not torch.equal(env.returns, G_before)                 # G still advances
    frozen = obs_w.normalize(tap.last)
    assert all(torch.equal(frozen[k], got[k]) for k in got)       # normalize() is the frozen form
    back = obs_w.unnormalize(got)
    assert all(torch.allclose(back[k], tap.last[k], rtol=1e-4, atol=1e-6) for k in got)


def test_composition_with_noise_and_flattening(twins):
    """``FlattenObservation(NormalizeObservation(SensorNoise(env)))`` is the flattening of the checker applied to the noisy dict the
    normaliser was handed (a tap between the two keeps it); ``NormalizeObservation(FlattenObservation(env))`` takes the single-tensor
    path."""
    _, inner = twins("rbc2d-batch")
    tap = Tap(SensorNoise(inner, 0.05, seed=77))
    env = FlattenObservation(NormalizeObservation(tap, clip=2.0, keys=["temperature", "velocity"]))
    chk = Checker(inner.observation_space, clip=2.0)

    def flat_of(noisy):
        chk.update({k: noisy[k] for k in ("temperature", "velocity")})
        return np.concatenate([chk.recs[k].apply(noisy[k].detach().cpu().numpy().reshape(3, -1), EPS, 2.0) for k in ("temperature", "velocity")],
                              axis=1)

    flat, _ = env.reset(seed=ENV_SEED)
    want = flat_of(tap.last)
    assert flat.shape == want.shape and np.all(np.abs(flat.cpu().numpy() - want) <= 2.0 ** -23 * np.maximum(1.0, np.abs(want)))
    a = _action(inner, 0.3)
    flat, *_ = env.step(a)
    want = flat_of(tap.last)
    assert np.all(np.abs(flat.cpu().numpy() - want) <= 2.0 ** -23 * np.maximum(1.0, np.abs(want)))
    assert float(flat.abs().max()) <= 2.0 and np.all(env.observation_space.high == 2.0)
    # the single-tensor path: NormalizeObservation outside FlattenObservation
    tap = Tap(FlattenObservation(inner))
    single = NormalizeObservation(tap, pool="key")
    chk1 = Checker(tap.observation_space, pooled=True)
    got, _ = single.reset(seed=ENV_SEED)
    chk1.update(tap.last)
    chk1.hold(got, tap.last, "flat reset")
    got, *_ = single.step(a)
    chk1.update(tap.last)
    chk1.hold(got, tap.last, "flat step")
    chk1.hold_records(single, "flat")
    assert isinstance(got, torch.Tensor) and got.shape == tap.last.shape and got.data_ptr() != tap.last.data_ptr()
    assert single.statistics["observation"][0] == 2 * tap.last.numel()


@pytest.mark.parametrize("pool", ["element", "key"])
def test_marl_channel_batch(twins, pool):
    """TCF, multi-agent, two envs: the rows are B x n_agents, the reward wrapper sees [B, n_agents]."""
    bare, inner = twins("tcf-marl-batch")
    assert bare.use_marl
    obs_w = NormalizeObservation(inner, pool=pool)
    env = NormalizeReward(obs_w, gamma=GAMMA, clip=5.0)
    chk = Checker(bare.observation_space, pooled=pool == "key")
    raw, _ = bare.reset(seed=ENV_SEED)
    got, _ = env.reset(seed=ENV_SEED)
    key = sorted(raw)[0]
    rows = _rows(raw[key], bare.observation_space.spaces[key])
    assert rows == 2 * bare.n_agents
    chk.update(raw)
    chk.hold(got, raw, f"marl {pool} reset")
    ret = R.ReturnRecord(rows, GAMMA)
    a = _action(bare, 0.2)
    raw, reward, *_ = bare.step(a)
    got, reward_w, *_ = env.step(a.clone())
    assert reward.shape == (2, bare.n_agents) and reward_w.shape == reward.shape and env.returns.shape == (rows,)
    chk.update(raw)
    chk.hold(got, raw, f"marl {pool} step")
    chk.hold_records(obs_w, f"marl {pool}")
    want = np.clip(ret.step(reward.cpu().numpy().reshape(-1), EPS).astype(np.float64), -5.0, 5.0)
    assert np.all(np.abs(reward_w.cpu().numpy().reshape(-1) - want) <= 2.0 ** -23 * np.maximum(1.0, np.abs(want)))
    D = raw[key].numel() // rows
    assert obs_w.statistics[key][0] == 2 * rows * (D if pool == "key" else 1) and env.statistics[0] == rows


def test_fp64_env(twins):
    bare, inner = twins("rbc2d-f64-batch")
    obs_w = NormalizeObservation(inner)
    env = NormalizeReward(obs_w, gamma=GAMMA)
    chk = Checker(bare.observation_space)
    raw, _ = bare.reset(seed=ENV_SEED)
    got, _ = env.reset(seed=ENV_SEED)
    chk.update(raw)
    chk.hold(got, raw, "f64 reset")
    a = _action(bare, 0.3)
    raw, reward, *_ = bare.step(a)
    got, reward_w, *_ = env.step(a.clone())
    assert all(got[k].dtype == torch.float64 for k in got) and reward_w.dtype == reward.dtype
    chk.update(raw)
    chk.hold(got, raw, "f64 step")
    chk.hold_records(obs_w, "f64")
    ret = R.ReturnRecord(2, GAMMA)
    g_max = _hold_reward(reward_w, reward, ret, "f64 reward")
    _hold_reward_record(env, ret, g_max, "f64 reward")
