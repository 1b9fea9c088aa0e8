"""CPU-side checks of the running normalisation: the NumPy checker against itself, the argument checks of
``fg_obs_normalize`` / ``fg_obs_return_normalize`` (which answer before any launch, without a GPU), the symbols, and the host logic of
``fluidgym_amd.wrappers.normalize`` on a small fake env."""
import ctypes

import numpy as np
import pytest
import torch

from fluidgym_amd import _lib as L
from fluidgym_amd import spaces
from fluidgym_amd.wrappers import FlattenObservation, NormalizeObservation, NormalizeReward, SensorNoise
from fluidgym_amd.wrappers.normalize import merge_records
from tests import obs_normalize_ref as R


# ------------------------------------------------------------------------------------------------ the checker
@pytest.mark.parametrize("pooled", [False, True])
def test_checker_streaming_merges_equal_two_pass_moments_of_the_concatenation(pooled):
    rng = np.random.default_rng(11)
    batches = [rng.uniform(-8, 8, (m, 7)) + 3.0 for m in (5, 1, 23)]
    rec = R.Record(pooled=pooled)
    for b in batches:
        rec.update(b)
    m, mean, m2 = R.batch_moments(np.concatenate(batches), axis=None if pooled else 0)
    assert rec.n == m == (29 * 7 if pooled else 29)
    assert np.max(np.abs(rec.mean - mean) / np.abs(mean)) <= 1e-13
    assert np.max(np.abs(rec.m2 - m2) / m2) <= 1e-13


def test_checker_empty_record_merged_with_a_batch_is_the_batch():
    x = np.random.default_rng(3).normal(size=(6, 4))
    m, mean, m2 = R.batch_moments(x)
    n, mean_r, m2_r = R.merge(0, None, None, m, mean, m2)
    assert n == 6 and np.array_equal(mean_r, mean) and np.array_equal(m2_r, m2)
    rows = R.Record().update(x, rows=[1, 4])
    assert rows.n == 2 and np.array_equal(rows.mean, x[[1, 4]].mean(0))


def test_checker_return_record():
    ret = R.ReturnRecord(3, 0.5)
    r = np.array([1.0, 2.0, 4.0], np.float32)
    y1 = ret.step(r)
    assert np.array_equal(ret.G, [1, 2, 4]) and ret.rec.n == 3
    ret.step(r)
    assert np.array_equal(ret.G, [1.5, 3, 6]) and ret.rec.n == 6
    var = np.var([1, 2, 4, 1.5, 3, 6])
    assert abs(ret.rec.m2 / 6 - var) < 1e-14 and y1.dtype == np.float32
    g = ret.G.copy()
    ret.step(r, update=False)
    assert ret.rec.n == 6 and np.array_equal(ret.G, 0.5 * g + r)


# ------------------------------------------------------------------------------------------------ the entries' argument checks
def _segment(**kw):
    base = dict(src=0x1000, dst=0x2000, src_stride=8, dst_stride=8, n=8, pooled=0, mean=0x3000, m2=0x4000)
    base.update(kw)
    return L.FgNormSegment(**base)


def _call(segs, n_seg=None, rows=2, dtype=0, n_before=4, n_add=None, row_list=None, n_rows_sel=0, update=1, epsilon=1e-8, clip=0.0):
    lib = L.load()
    arr = (L.FgNormSegment * max(len(segs), 1))(*segs) if segs is not None else None
    if n_add is None:
        n_add = (n_rows_sel if row_list else rows) if update else 0
    rc = lib.fg_obs_normalize(arr, len(segs) if n_seg is None else n_seg, rows, dtype, n_before, n_add,
                              ctypes.c_void_p(row_list) if row_list else None, n_rows_sel, update, epsilon, clip, None)
    return rc, lib.fg_last_error().decode()


@pytest.mark.parametrize("what, kw, word", [
    ("no segments", dict(segs=None, n_seg=1), "null"),
    ("n_seg 0", dict(n_seg=0), "n_seg"),
    ("n_seg 9", dict(segs=[_segment()] * 9), "n_seg"),
    ("rows 0", dict(rows=0, n_add=0), "rows"),
    ("rows 65536", dict(rows=65536), "rows"),
    ("dtype", dict(dtype=2), "dtype"),
    ("null src", dict(segs=[_segment(src=None)]), "null"),
    ("null dst", dict(segs=[_segment(), _segment(dst=None)]), "segment 1"),
    ("null mean", dict(segs=[_segment(mean=None)]), "null"),
    ("null m2", dict(segs=[_segment(m2=None)]), "null"),
    ("n 0", dict(segs=[_segment(n=0)]), "n = 0"),
    ("n above 2^26", dict(segs=[_segment(n=(1 << 26) + 1, src_stride=1 << 27, dst_stride=1 << 27)]), "2^26"),
    ("src stride", dict(segs=[_segment(src_stride=7)]), "stride"),
    ("dst stride", dict(segs=[_segment(dst_stride=7)]), "stride"),
    ("n_add is not the rows", dict(n_add=3), "n_add"),
    ("n_add is not the listed rows", dict(rows=4, row_list=0x5000, n_rows_sel=2, n_add=4), "n_add"),
    ("n_add of a frozen call", dict(update=0, n_add=2), "n_add"),
    ("n_before negative", dict(n_before=-1), "n_before"),
    ("frozen and empty", dict(update=0, n_before=0), "update = 0"),
    ("n_rows_sel 0", dict(row_list=0x5000, n_rows_sel=0), "n_rows_sel"),
    ("n_rows_sel above rows", dict(row_list=0x5000, n_rows_sel=3), "n_rows_sel"),
    ("epsilon 0", dict(epsilon=0.0), "epsilon"),
    ("epsilon negative", dict(epsilon=-1e-8), "epsilon"),
])
def test_normalize_entry_refuses_bad_arguments_without_a_gpu(what, kw, word):
    """Every refusal is a status code with a message, before any launch: the pointers here are never dereferenced."""
    args = dict(segs=[_segment()])
    args.update(kw)
    rc, msg = _call(**args)
    assert rc == L.FG_ERR_INVALID_ARG and "fg_obs_normalize" in msg and word in msg, (what, rc, msg)


def _call_return(reward=0x1000, out=0x2000, G=0x3000, stats=0x4000, rows=2, dtype=0, gamma=0.99, n_before=4, epsilon=1e-8, clip=0.0,
                 update=1):
    lib = L.load()
    p = ctypes.c_void_p
    rc = lib.fg_obs_return_normalize(p(reward), p(out), p(G), p(stats), rows, dtype, gamma, n_before, epsilon, clip, update, None)
    return rc, lib.fg_last_error().decode()


@pytest.mark.parametrize("what, kw, word", [
    ("null reward", dict(reward=None), "null"),
    ("null out", dict(out=None), "null"),
    ("null G", dict(G=None), "null"),
    ("null stats", dict(stats=None), "null"),
    ("rows 0", dict(rows=0), "rows"),
    ("rows 65536", dict(rows=65536), "rows"),
    ("dtype", dict(dtype=-1), "dtype"),
    ("gamma negative", dict(gamma=-0.1), "gamma"),
    ("gamma above 1", dict(gamma=1.01), "gamma"),
    ("n_before negative", dict(n_before=-2), "n_before"),
    ("frozen and empty", dict(update=0, n_before=0), "update = 0"),
    ("epsilon 0", dict(epsilon=0.0), "epsilon"),
])
def test_return_entry_refuses_bad_arguments_without_a_gpu(what, kw, word):
    rc, msg = _call_return(**kw)
    assert rc == L.FG_ERR_INVALID_ARG and "fg_obs_return_normalize" in msg and word in msg, (what, rc, msg)


def test_entries_belong_to_the_fp32_library_only():
    import os
    import re
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fluidgym_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("fg_obs_normalize", "fg_obs_return_normalize"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in L.SIGNATURES and name not in L.SIGNATURES_F64
        assert hasattr(L.load(), name) and not hasattr(L.load_f64(), name)
    assert ctypes.sizeof(L.FgNormSegment) == 56
    assert len(L.SIGNATURES["fg_obs_normalize"][1]) == 12 and len(L.SIGNATURES["fg_obs_return_normalize"][1]) == 12


# ------------------------------------------------------------------------------------------------ host logic on a fake env
class FakeEnv:
    """The members the wrappers touch, on CPU tensors."""

    def __init__(self, num_envs=2, box=False):
        self.num_envs, self._box, self.state_set = num_envs, box, None

    cuda_device = property(lambda self: torch.device("cpu"))
    use_marl = property(lambda self: False)

    @property
    def observation_space(self):
        if self._box:
            return spaces.Box(low=-1.0, high=1.0, shape=(5,), dtype=np.float32)
        return spaces.Dict({
            "temperature": spaces.Box(low=1.0, high=2.0, shape=(2, 3), dtype=np.float32),
            "velocity": spaces.Box(low=-np.inf, high=np.inf, shape=(2, 2, 3), dtype=np.float32),
            "pressure": spaces.Box(low=-5.0, high=5.0, shape=(2, 3), dtype=np.float64),
        })

    def _obs(self):
        if self._box:
            return torch.zeros(self.num_envs, 5)
        return {k: torch.zeros((self.num_envs,) + tuple(s.shape)) for k, s in self.observation_space.spaces.items()}

    def reset(self, seed=None, randomize=None):
        return self._obs(), {}

    def reset_envs(self, envs, randomize=None):
        return self._obs()

    def step(self, action):
        return self._obs(), torch.zeros(self.num_envs), False, False, {}

    def get_state(self):
        return {"t": 0}

    def set_state(self, state):
        self.state_set = dict(state)


def _fill(w, rng, n):
    """A record put into ``w`` through its state entry (there is no CPU kernel to produce one)."""
    entry = {"n": n, "mean": {}, "M2": {}}
    for k, size in w._sizes.items():
        slots = 1 if w._pooled else size
        entry["mean"][k] = torch.from_numpy(rng.normal(size=slots))
        entry["M2"][k] = torch.from_numpy(rng.uniform(1.0, 2.0, size=slots) * n)
    w._set_record_entry(entry)
    return entry


def test_observation_space_bounds_and_arguments():
    env = FakeEnv()
    w = NormalizeObservation(env, clip=5.0, keys=["velocity", "pressure"])
    sp = w.observation_space
    assert list(sp.spaces) == ["temperature", "velocity", "pressure"]
    assert sp.spaces["temperature"] is env.observation_space.spaces["temperature"] or np.all(sp.spaces["temperature"].low == 1.0)
    for k in ("velocity", "pressure"):
        ref = env.observation_space.spaces[k]
        assert sp.spaces[k].shape == ref.shape and sp.spaces[k].dtype == ref.dtype
        assert np.all(sp.spaces[k].low == -5.0) and np.all(sp.spaces[k].high == 5.0)
    free = NormalizeObservation(env).observation_space
    assert all(np.all(np.isneginf(s.low)) and np.all(np.isposinf(s.high)) for s in free.spaces.values())
    box = NormalizeObservation(FakeEnv(box=True), clip=2.0).observation_space
    assert isinstance(box, spaces.Box) and box.shape == (5,) and np.all(box.high == 2.0) and box.dtype == np.float32
    with pytest.raises(ValueError, match="pool"):
        NormalizeObservation(env, pool="row")
    with pytest.raises(ValueError, match="Key 'vorticity'"):
        NormalizeObservation(env, keys=["vorticity"])
    with pytest.raises(ValueError, match="epsilon"):
        NormalizeObservation(env, epsilon=0.0)
    with pytest.raises(ValueError, match="clip"):
        NormalizeReward(env, clip=-1.0)
    with pytest.raises(ValueError, match="gamma"):
        NormalizeReward(env, gamma=1.5)
    with pytest.raises(ValueError, match="keys"):
        NormalizeObservation(FakeEnv(box=True), keys=["a"])


def test_cpu_tensors_are_refused_and_the_switch_is_independent_of_the_mode():
    env = FakeEnv()
    w = NormalizeObservation(env)
    with pytest.raises(L.NativeLibraryError, match="no CPU path"):
        w.reset(seed=0)
    with pytest.raises(L.NativeLibraryError, match="no CPU path"):
        w.step(None)
    with pytest.raises(L.NativeLibraryError, match="no CPU path"):
        w.reset_envs([0])
    with pytest.raises(L.NativeLibraryError, match="no CPU path"):
        NormalizeReward(env).step(None)
    with pytest.raises(L.NativeLibraryError, match="no CPU path"):
        NormalizeObservation(FakeEnv(box=True)).reset()
    assert w.updating
    w.freeze()
    assert not w.updating
    with pytest.raises(RuntimeError, match="empty"):     # frozen with n == 0: before any launch
        w.step(None)
    with pytest.raises(RuntimeError, match="empty"):
        w.normalize(env._obs())
    r = NormalizeReward(env)
    r.freeze()
    with pytest.raises(RuntimeError, match="empty"):
        r.step(None)
    w.unfreeze()
    assert w.updating and w.statistics == {}


@pytest.mark.parametrize("pool", ["element", "key"])
def test_save_load_round_trip_and_merge_against_the_checker(tmp_path, pool):
    rng = np.random.default_rng(5)
    env = FakeEnv()
    a, b = NormalizeObservation(env, pool=pool), NormalizeObservation(env, pool=pool)
    ea, eb = _fill(a, rng, 7), _fill(b, rng, 12)
    path = tmp_path / "record.npz"
    a.save(path)
    c = NormalizeObservation(env, pool=pool)
    c.load(path)
    assert c._n == 7 and set(c._mean) == set(a._mean)
    for k in a._mean:
        assert torch.equal(c._mean[k], a._mean[k]) and torch.equal(c._m2[k], a._m2[k]) and c._mean[k].dtype == torch.float64
    with pytest.raises(ValueError, match="pool"):
        NormalizeObservation(env, pool="key" if pool == "element" else "element").load(path)
    a.merge(b)
    assert a._n == 19
    for k, size in a._sizes.items():
        scale = size if pool == "key" else 1
        n, mean, m2 = R.merge(7 * scale, ea["mean"][k].numpy(), ea["M2"][k].numpy(), 12 * scale, eb["mean"][k].numpy(), eb["M2"][k].numpy())
        count, s_mean, s_var = a.statistics[k]
        assert count == n
        np.testing.assert_allclose(s_mean.numpy(), mean, rtol=1e-15, atol=0)
        np.testing.assert_allclose(s_var.numpy(), m2 / n, rtol=1e-15, atol=0)
    empty = NormalizeObservation(env, pool=pool)
    empty.merge(b)                                           # an empty record merged with another is the other
    assert empty._n == 12 and all(torch.equal(empty._mean[k], b._mean[k]) and torch.equal(empty._m2[k], b._m2[k]) for k in b._mean)
    b.merge(NormalizeObservation(env, pool=pool))            # and the other way round nothing moves
    assert b._n == 12 and all(torch.equal(b._mean[k], eb["mean"][k]) for k in b._mean)
    with pytest.raises(ValueError, match="merge"):
        a.merge(NormalizeObservation(env, pool=pool, keys=["velocity"]))
    # unnormalize inverts the record's map (plain torch on whatever device the tensors are on)
    y = {k: torch.from_numpy(rng.normal(size=(2,) + tuple(s.shape))).to(torch.float32) for k, s in env.observation_space.spaces.items()}
    x = b.unnormalize(y)
    for k, size in b._sizes.items():
        count = 12 * (size if pool == "key" else 1)
        want = y[k].reshape(2, -1).double().numpy() * np.sqrt(b._m2[k].numpy() / count + 1e-8) + b._mean[k].numpy()
        np.testing.assert_allclose(x[k].reshape(2, -1).numpy(), want, rtol=2e-7)


def test_reward_record_save_load_and_merge(tmp_path):
    env = FakeEnv()
    a, b = NormalizeReward(env), NormalizeReward(env)
    a._set_record_entry({"n": 4, "mean": torch.tensor(1.5, dtype=torch.float64), "M2": torch.tensor(3.0, dtype=torch.float64), "G": None})
    b._set_record_entry({"n": 6, "mean": torch.tensor(-0.5, dtype=torch.float64), "M2": torch.tensor(8.0, dtype=torch.float64),
                         "G": torch.ones(2, dtype=torch.float64)})
    a.save(tmp_path / "r.npz")
    c = NormalizeReward(env)
    c.load(tmp_path / "r.npz")
    assert c.statistics[0] == 4 and float(c.statistics[1]) == 1.5 and float(c.statistics[2]) == 0.75 and c.returns is None
    a.merge(b)
    n, mean, m2 = R.merge(4, np.float64(1.5), np.float64(3.0), 6, np.float64(-0.5), np.float64(8.0))
    assert a.statistics[0] == n == 10 and float(a.statistics[1]) == float(mean) and abs(float(a.statistics[2]) - m2 / 10) < 1e-15
    r = torch.tensor([2.0, -4.0])
    scaled = a.normalize(r)
    np.testing.assert_allclose(scaled.numpy(), r.numpy() / np.sqrt(m2 / 10 + 1e-8), rtol=2e-7)
    np.testing.assert_allclose(a.unnormalize(scaled).numpy(), r.numpy(), rtol=3e-7)
    assert torch.equal(b.returns, torch.ones(2, dtype=torch.float64))


def test_merge_records_helper_is_the_update_rule():
    ma, mb = torch.tensor([1.0, 2.0], dtype=torch.float64), torch.tensor([3.0, -2.0], dtype=torch.float64)
    sa, sb = torch.tensor([4.0, 1.0], dtype=torch.float64), torch.tensor([0.5, 2.5], dtype=torch.float64)
    mean, m2 = merge_records(3, ma, sa, 5, mb, sb)
    n, want_mean, want_m2 = R.merge(3, ma.numpy(), sa.numpy(), 5, mb.numpy(), sb.numpy())
    assert n == 8 and np.array_equal(mean.numpy(), want_mean) and np.array_equal(m2.numpy(), want_m2)


def test_state_keys_of_nested_normalisers_with_a_noise_wrapper_between_them():
    """Each wrapper keeps its record under a key of its own, numbered from the inside out, takes its own entry out in ``set_state`` and
    hands the rest on; the entries are clones."""
    env = FakeEnv()
    inner = NormalizeObservation(env)
    outer = NormalizeObservation(SensorNoise(inner, sigma=0.1, seed=1), pool="key")
    top = NormalizeReward(NormalizeReward(outer, gamma=0.5))
    rng = np.random.default_rng(9)
    _fill(inner, rng, 3), _fill(outer, rng, 5)
    state = top.get_state()
    assert set(state) == {"t", "obs_normalizer", "sensor_noise_counters", "obs_normalizer#1", "reward_normalizer", "reward_normalizer#1"}
    assert state["obs_normalizer"]["n"] == 3 and state["obs_normalizer#1"]["n"] == 5
    assert set(state["obs_normalizer"]) == {"n", "mean", "M2"} and set(state["reward_normalizer"]) == {"n", "mean", "M2", "G"}
    assert state["obs_normalizer"]["mean"]["velocity"].shape == (12,) and state["obs_normalizer#1"]["mean"]["velocity"].shape == (1,)
    kept = state["obs_normalizer"]["mean"]["velocity"].clone()
    inner._mean["velocity"] += 1.0                           # the entry is a clone
    assert torch.equal(state["obs_normalizer"]["mean"]["velocity"], kept)
    inner._n, outer._n = 0, 0
    top.set_state(state)
    assert env.state_set == {"t": 0} and inner._n == 3 and outer._n == 5
    assert torch.equal(inner._mean["velocity"], kept)
    state["obs_normalizer"]["mean"]["velocity"] += 1.0       # and set_state keeps clones too
    assert torch.equal(inner._mean["velocity"], kept)
    with pytest.raises(KeyError, match="obs_normalizer"):
        outer.set_state({"t": 0, "sensor_noise_counters": None})
    with pytest.raises(KeyError, match="reward_normalizer"):
        top.set_state({"t": 0})
    assert isinstance(FlattenObservation(inner).observation_space, spaces.Box)      # composes with the other wrappers
