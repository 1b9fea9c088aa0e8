"""CPU-side checks of ``fluidgym_amd.wrappers`` and of the noise stream's definition: the NumPy checker's Philox
against the published known answers, its fp32 normal numbers against fp64 Box-Muller and a unit normal's moments, the wrapper logic on
a small fake env, and the argument checks of ``fg_obs_noise_add`` (which answer before any launch, without a GPU)."""
import ctypes

import numpy as np
import pytest
import torch

from fluidgym_amd import _lib as L
from fluidgym_amd import spaces
from fluidgym_amd.types import FLUID_ENV_LIKE_MEMBERS, FluidEnvLike
from fluidgym_amd.wrappers import ActionNoise, FlattenObservation, FluidWrapper, ObsExtraction, SensorNoise
from fluidgym_amd.wrappers.util import flatten_box_space, flatten_dict_space
from tests import obs_noise_ref as R

DRAW_SEED = 20240229          # the one fixed seed of the 2^20 draws
N_DRAWS = 1 << 20


# ------------------------------------------------------------------------------------------------ the stream's definition
@pytest.mark.parametrize("counter, key, words", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, words):
    out = R.philox4x32_10([np.uint64(c) for c in counter], [np.uint64(k) for k in key])
    assert " ".join("%08x" % int(w) for w in out) == words


@pytest.fixture(scope="module")
def draws():
    """2^20 word pairs of one fixed seed (2^19 Philox blocks of the checker itself), then every pair of the edge words."""
    w = R.philox4x32_10((np.arange(N_DRAWS // 2, dtype=np.uint64), np.uint64(0), np.uint64(0), np.uint64(0)),
                        (np.uint64(DRAW_SEED), np.uint64(0)))
    w0, w1 = np.concatenate([w[0], w[2]]), np.concatenate([w[1], w[3]])
    e0, e1 = np.meshgrid(R.EDGE_WORDS, R.EDGE_WORDS)
    w0, w1 = np.concatenate([w0, e0.ravel()]), np.concatenate([w1, e1.ravel()])
    return w0, w1, R.normal_pair(w0, w1)


def test_normals_against_fp64_box_muller(draws):
    """The design condition of the approximation: within 2e-6 max(1, |z|) of fp64 Box-Muller of the same words, every value finite."""
    w0, w1, (z0, z1) = draws
    x0, x1 = R.box_muller_f64(w0, w1)
    assert z0.dtype == np.float32 and z1.dtype == np.float32
    assert np.isfinite(z0).all() and np.isfinite(z1).all()
    dev = max(float(np.max(np.abs(z0 - x0) / np.maximum(1.0, np.abs(x0)))), float(np.max(np.abs(z1 - x1) / np.maximum(1.0, np.abs(x1)))))
    print(f"largest deviation from fp64 Box-Muller: {dev:.3e};  max |z| = {max(np.abs(z0).max(), np.abs(z1).max()):.3f}")
    assert dev <= 2e-6


def test_normals_have_unit_normal_moments(draws):
    """2^20 pairs = 2^21 values; the bounds are five standard errors of a unit normal's moments at 2^20 values (sqrt(1 / n),
    sqrt(2 / n), sqrt(15 / n), sqrt(96 / n)), held by the z0 and by the z1 of the seeded draws separately."""
    _, _, (z0, z1) = draws
    for z in (z0[:N_DRAWS].astype(np.float64), z1[:N_DRAWS].astype(np.float64)):
        m1, m2, m3, m4 = z.mean(), z.var(), (z ** 3).mean(), (z ** 4).mean()
        print(f"mean {m1:+.3e}  var-1 {m2 - 1:+.3e}  third {m3:+.3e}  fourth-3 {m4 - 3:+.3e}")
        assert abs(m1) <= 4.9e-3
        assert abs(m2 - 1.0) <= 6.9e-3
        assert abs(m3) <= 1.9e-2
        assert abs(m4 - 3.0) <= 4.8e-2


def test_checker_rows_are_independent_of_the_launch():
    """A row's numbers depend on its id and counters only: rows [5, 2] of a six-row launch, and the quad structure of a row."""
    c = np.array([[3, 1], [3, 2], [4, 0], [1, 7], [2, 2], [9, 9]])
    src = np.zeros((6, 11), np.float32)
    full = R.noise_add([dict(src=src, tag=3, sigma=1.0)], 6, c, None, 77, 0)[0]
    part = R.noise_add([dict(src=src[:2], tag=3, sigma=1.0)], 2, c[[5, 2]], [5, 2], 77, 0)[0]
    assert np.array_equal(part.view(np.uint32), full[[5, 2]].view(np.uint32))
    assert np.array_equal(R.normals(5, 3, 1, 3, 2, 77), full[1, :5])
    assert not np.array_equal(full[0], full[1])
    assert not np.array_equal(R.normals(11, 4, 1, 3, 2, 77), full[1])


# ------------------------------------------------------------------------------------------------ a fake FluidEnvLike
class FakeEnv:
    """The protocol's members on CPU tensors: observations are counters one can recognise, ``step`` records the action it got."""

    def __init__(self, num_envs=None, use_marl=False, n_agents=3, dtype=torch.float32):
        self._num_envs, self._marl, self._n_agents, self._dtype = num_envs, use_marl, n_agents, dtype
        self._t = 0
        self.last_action = None
        self.resets = []
        self.state_set = None

    num_envs = property(lambda self: 1 if self._num_envs is None else self._num_envs)
    use_marl = property(lambda self: self._marl)
    n_agents = property(lambda self: self._n_agents if self._marl else 1)
    episode_length = property(lambda self: 5)
    metrics = property(lambda self: ["m"])
    cuda_device = property(lambda self: torch.device("cpu"))
    differentiable = property(lambda self: False)
    only_here = "batch-only member"

    @property
    def action_space(self):
        return spaces.Box(low=-1.0, high=1.0, shape=(1,) if self._marl else (4, 1), dtype=np.float32)

    @property
    def observation_space(self):
        return spaces.Dict({
            "temperature": spaces.Box(low=1.0, high=2.0, shape=(2, 3), dtype=np.float32),
            "velocity": spaces.Box(low=-np.inf, high=np.inf, shape=(2, 2, 3), dtype=np.float32),
            "pressure": spaces.Box(low=-np.inf, high=np.inf, shape=(2, 3), dtype=np.float32),
        })

    def _lead(self):
        return (() if self._num_envs is None else (self._num_envs,)) + ((self._n_agents,) if self._marl else ())

    def _obs(self):
        out = {}
        for i, (k, s) in enumerate(self.observation_space.spaces.items()):
            shape = self._lead() + tuple(s.shape)
            out[k] = (torch.arange(int(np.prod(shape)), dtype=self._dtype).reshape(shape) + 1000 * i + 100000 * self._t)
        return out

    def reset(self, seed=None, randomize=None):
        self.resets.append((seed, randomize))
        self._t = 0
        return self._obs(), {}

    def reset_envs(self, envs, randomize=None):
        return self._obs()

    def step(self, action):
        self.last_action = action
        self._t += 1
        return self._obs(), torch.zeros(self._lead()), False, self._t >= 5, {"m": torch.tensor(1.0)}

    def seed(self, seed):
        self.seeded = seed

    def render(self, save=False, render_3d=False, filename=None, output_path=None):
        return ("render", save, render_3d, filename, output_path)

    def sample_action(self):
        return torch.zeros(self._lead() + tuple(self.action_space.shape))

    def get_state(self):
        return {"t": self._t}

    def set_state(self, state):
        self.state_set = dict(state)
        self._t = state["t"]

    def train(self):
        self.mode = "train"

    def val(self):
        self.mode = "val"

    def test(self):
        self.mode = "test"

    def save_gif(self, filename, output_path=None):
        self.gif = (filename, output_path)

    def load_initial_domain(self, idx, mode=None):
        self.loaded = (idx, mode)

    def get_uncontrolled_episode_metrics(self):
        return None

    def detach(self):
        self.detached = True


def test_delegation_and_unwrapped_through_two_levels():
    env = FakeEnv(num_envs=2)
    w = FluidWrapper(FluidWrapper(env))
    assert isinstance(w, FluidEnvLike) and all(hasattr(w, m) for m in FLUID_ENV_LIKE_MEMBERS)
    assert w.unwrapped is env and w._env.unwrapped is env
    assert w.num_envs == 2 and w.only_here == "batch-only member"       # not protocol members: __getattr__
    with pytest.raises(AttributeError):
        w.no_such_member
    assert (w.use_marl, w.n_agents, w.episode_length, w.metrics, w.differentiable) == (False, 1, 5, ["m"], False)
    assert w.cuda_device == torch.device("cpu")
    assert w.action_space.shape == (4, 1) and set(w.observation_space.spaces) == {"temperature", "velocity", "pressure"}
    obs, info = w.reset(seed=3, randomize=True)
    assert env.resets == [(3, True)] and info == {}
    a = w.sample_action()
    assert w.step(a)[0]["pressure"].shape == (2, 2, 3) and env.last_action is a
    w.seed(9), w.val(), w.save_gif("f", output_path="p"), w.load_initial_domain(idx=2), w.detach()
    assert (env.seeded, env.mode, env.gif, env.loaded, env.detached) == (9, "val", ("f", "p"), (2, None), True)
    assert w.render(save=True, filename="x") == ("render", True, False, "x", None)
    assert w.get_uncontrolled_episode_metrics() is None
    assert w.get_state() == {"t": 1}
    w.set_state({"t": 4})
    assert env._t == 4
    assert torch.equal(w.reset_envs([0])["temperature"], env._obs()["temperature"])     # a batch-only member passes through
    import inspect
    assert list(inspect.signature(FluidWrapper.reset).parameters) == ["self", "seed", "randomize"]
    assert list(inspect.signature(FluidWrapper.render).parameters) == ["self", "save", "render_3d", "filename", "output_path"]


def test_obs_extraction_errors_space_and_filter():
    env = FakeEnv()
    with pytest.raises(ValueError, match="Keys list must be non-empty or None."):
        ObsExtraction(env, [])
    with pytest.raises(ValueError, match="Key 'vorticity' not found in observation space."):
        ObsExtraction(env, ["velocity", "vorticity"])
    boxed = FluidWrapper(env)
    boxed.__class__ = type("Boxed", (FluidWrapper,), {"observation_space": property(lambda s: spaces.Box(0.0, 1.0, shape=(3,)))})
    with pytest.raises(ValueError, match="only supports Dict observation spaces"):
        ObsExtraction(boxed, ["velocity"])
    w = ObsExtraction(env, ["pressure", "temperature"])
    assert isinstance(w.observation_space, spaces.Dict) and list(w.observation_space.spaces) == ["pressure", "temperature"]
    assert w.observation_space.spaces["pressure"].shape == (2, 3)
    obs, _ = w.reset(seed=0)
    assert list(obs) == ["pressure", "temperature"]
    assert list(w.step(env.sample_action())[0]) == ["pressure", "temperature"]
    assert list(w.reset_envs([0])) == ["pressure", "temperature"]
    assert w.unwrapped is env


@pytest.mark.parametrize("num_envs, marl, lead", [(None, False, ()), (None, True, (3,)), (4, False, (4,)), (2, True, (2, 3))])
def test_flatten_observation_shapes_space_and_originals(num_envs, marl, lead):
    env = FakeEnv(num_envs=num_envs, use_marl=marl)
    w = FlattenObservation(env)
    D = 6 + 12                       # temperature, then velocity; pressure is not flattened (the reference's key list)
    space = w.observation_space
    assert isinstance(space, spaces.Box) and space.shape == (D,) and space.dtype == np.float32
    assert np.all(space.low[:6] == 1.0) and np.all(space.high[:6] == 2.0) and np.all(np.isinf(space.low[6:]))
    flat, info = w.reset(seed=0)
    raw = env._obs()
    assert flat.shape == lead + (D,)
    want = torch.cat([raw["temperature"].reshape(lead + (-1,)), raw["velocity"].reshape(lead + (-1,))], dim=-1)
    assert torch.equal(flat, want)
    assert set(info) == {"original_temperature", "original_velocity", "original_pressure"}
    assert torch.equal(info["original_velocity"], raw["velocity"])
    flat, _, _, _, info = w.step(env.sample_action())
    assert flat.shape == lead + (D,) and torch.equal(info["original_pressure"], env._obs()["pressure"]) and "m" in info
    assert w.reset_envs([0]).shape == lead + (D,)
    # a row of the flat observation is that row's items, whatever the batch around it
    row = tuple(0 for _ in lead)
    assert torch.equal(flat[row][:6], env._obs()["temperature"][row].reshape(-1))


def test_flatten_observation_keeps_originals_in_per_env_info_lists():
    """``ParallelFluidEnv`` returns one info dict per env: each keeps its own env's un-flattened tensors."""
    class Listed(FluidWrapper):
        def reset(self, seed=None, randomize=None):
            obs, _ = self._env.reset(seed=seed, randomize=randomize)
            return obs, [{"env": e} for e in range(self._env.num_envs)]

    env = FakeEnv(num_envs=3)
    flat, infos = FlattenObservation(Listed(env)).reset(seed=0)
    assert flat.shape == (3, 18) and [i["env"] for i in infos] == [0, 1, 2]
    assert all(torch.equal(infos[e]["original_velocity"], env._obs()["velocity"][e]) for e in range(3))


def test_flatten_spaces():
    box = flatten_box_space(spaces.Box(low=np.array([[0.0, 1.0], [2.0, 3.0]]), high=np.array([[4.0, 5.0], [6.0, 7.0]]), dtype=np.float32))
    assert box.shape == (4,) and list(box.low) == [0, 1, 2, 3] and list(box.high) == [4, 5, 6, 7] and box.dtype == np.float32
    d = spaces.Dict({"a": spaces.Box(0.0, 1.0, shape=(2,), dtype=np.float32), "b": spaces.Box(-2.0, 2.0, shape=(1, 3), dtype=np.float64)})
    flat = flatten_dict_space(d)
    assert flat.shape == (5,) and flat.dtype == np.float64 and list(flat.low) == [0, 0, -2, -2, -2]
    only_a = flatten_dict_space(d, keys=["a"])
    assert only_a.shape == (2,) and only_a.dtype == np.float32
    assert flatten_dict_space(d, keys=["b", "a"]).low[0] == -2
    with pytest.raises(TypeError, match="Expected spaces.Dict"):
        flatten_dict_space(d.spaces["a"])
    with pytest.raises(KeyError, match="Key 'c' not found in the Dict space."):
        flatten_dict_space(d, keys=["c"])
    with pytest.raises(TypeError, match="Only Box subspaces supported, but key 'n'"):
        flatten_dict_space(spaces.Dict({"n": spaces.Dict({"a": d.spaces["a"]})}))
    with pytest.raises(ValueError, match="contains no Box subspaces"):
        flatten_dict_space(d, keys=[])
    with pytest.raises(ValueError, match="only supports Dict observation spaces"):
        FlattenObservation(FlattenObservation(FakeEnv()))


def test_noise_wrappers_refuse_the_cpu_at_the_first_observation_and_carry_state_keys():
    """Construction touches nothing; the first observation on a CPU device raises the package's error (there is no CPU path).  The state
    entries of nested wrappers coexist and each takes its own out before handing the rest on."""
    env = FakeEnv(num_envs=2)
    s = SensorNoise(ActionNoise(SensorNoise(env, 0.1, seed=1), sigma=0.2, seed=2, first_row=4), sigma=0.3, seed=3)
    assert s.unwrapped is env and s.num_envs == 2
    with pytest.raises(L.NativeLibraryError, match="no CPU path"):
        s.reset(seed=0)
    state = s.get_state()
    assert set(state) == {"t", "sensor_noise_counters", "action_noise_counters", "sensor_noise_counters#1"}
    s.set_state(state)
    assert env.state_set == {"t": 0}
    with pytest.raises(KeyError, match="sensor_noise_counters"):
        s.set_state({"t": 0})
    with pytest.raises(RuntimeError, match="reset"):
        ActionNoise(env, 0.1, 0).step(env.sample_action())
    with pytest.raises(ValueError, match="first_row"):
        SensorNoise(env, 0.1, 0, first_row=-1)
    import inspect
    for cls in (SensorNoise, ActionNoise):
        p = inspect.signature(cls.__init__).parameters
        assert list(p) == ["self", "env", "sigma", "seed", "first_row"] and p["first_row"].kind is p["first_row"].KEYWORD_ONLY


# ------------------------------------------------------------------------------------------------ the entry's argument checks
def _segment(**kw):
    base = dict(src=0x1000, dst=0x2000, src_stride=8, dst_stride=8, n=8, tag=0, sigma=1.0)
    base.update(kw)
    return L.FgNoiseSegment(**base)


def _call(segs, n_seg=None, rows=2, dtype=0, counters=0x3000):
    lib = L.load()
    arr = (L.FgNoiseSegment * max(len(segs), 1))(*segs) if segs is not None else None
    rc = lib.fg_obs_noise_add(arr, len(segs) if n_seg is None else n_seg, rows, dtype, 5, ctypes.c_void_p(counters), None, None)
    return rc, lib.fg_last_error().decode()


@pytest.mark.parametrize("what, kw, word", [
    ("no segments", dict(segs=None, n_seg=1), "null"),
    ("no counters", dict(counters=None), "null"),
    ("n_seg 0", dict(n_seg=0), "n_seg"),
    ("n_seg 9", dict(segs=[_segment()] * 9), "n_seg"),
    ("rows 0", dict(rows=0), "rows"),
    ("rows 65536", dict(rows=65536), "rows"),
    ("dtype", dict(dtype=2), "dtype"),
    ("null src", dict(segs=[_segment(src=None)]), "null"),
    ("null dst", dict(segs=[_segment(), _segment(dst=None)]), "segment 1"),
    ("n 0", dict(segs=[_segment(n=0)]), "n = 0"),
    ("n above 2^26", dict(segs=[_segment(n=(1 << 26) + 1, src_stride=1 << 27, dst_stride=1 << 27)]), "2^26"),
    ("tag 256", dict(segs=[_segment(tag=256)]), "tag"),
    ("src stride", dict(segs=[_segment(src_stride=7)]), "stride"),
    ("dst stride", dict(segs=[_segment(dst_stride=7)]), "stride"),
])
def test_entry_refuses_bad_arguments_without_a_gpu(what, kw, word):
    """Every refusal is a status code with a message, before any launch: the pointers here are never dereferenced."""
    args = dict(segs=[_segment()])
    args.update(kw)
    rc, msg = _call(**args)
    assert rc == L.FG_ERR_INVALID_ARG and "fg_obs_noise_add" in msg and word in msg, (what, rc, msg)


def test_entry_belongs_to_the_fp32_library_only():
    assert "fg_obs_noise_add" in L.SIGNATURES and "fg_obs_noise_add" not in L.SIGNATURES_F64
    assert ctypes.sizeof(L.FgNoiseSegment) == 48
    assert not hasattr(L.load_f64(), "fg_obs_noise_add")
