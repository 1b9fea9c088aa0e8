"""``fg_baseline_opposition`` / ``fg_baseline_pd`` and the controllers of ``fluidgym_amd/baselines.py`` on the GPU, held to the NumPy fp64
restatement (``tests/baselines_ref.py``).  No long simulation: the fields are seeded normal numbers.

Bounds (derived, not measured).  The kernels sum in fp64 and round once to the field type; the restatement is fp64 throughout.
Opposition control, at most 4096 cells per plane, ``|action| <= 2 alpha max|v|``: fp32 ``1 ulp_fp32(max|v|)`` (half an ulp one binade
up), fp64 ``4096 * 2^-52 max|v|``.  PD control: ``|action| <= S max|v|`` with ``S = kp + 2 kd / dt`` (both ``E`` of the derivative
carry their own error), the term count is the cells of one heater column: fp32 ``1 ulp_fp32(S max|v|)``, fp64
``cells * 2^-52 S max|v|``."""
import ctypes

import numpy as np
import pytest
import torch

import fluidgym_amd
from fluidgym_amd import _lib as L
from fluidgym_amd.baselines import OppositionControl, PDControl, run_baseline_episodes
from fluidgym_amd.types import EnvMode
from tests import baselines_ref as R

pytestmark = pytest.mark.gpu

DTYPES = {"fp32": torch.float32, "fp64": torch.float64}


def _bound(dtype, vmax, terms, scale=1.0):
    if dtype == torch.float32:
        return float(np.spacing(np.float32(scale * vmax)))
    return terms * 2.0 ** -52 * scale * vmax


def _normal(shape, seed, dtype, device, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (scale * torch.randn(shape, generator=g, dtype=torch.float64)).to(dtype).to(device)


# ------------------------------------------------------------------------------------------------ the kernels alone, every form
def _component_view(B, nz, ny, nx, dtype, off, seed):
    """Component 1 of a ``[B, 3, nz, ny, nx]`` field that starts ``off`` reals into its allocation (off = 1: no 16-byte alignment)."""
    cells = nz * ny * nx
    buf = torch.zeros(B * 3 * cells + 4, dtype=dtype, device="cuda")
    field = buf[off: off + B * 3 * cells].view(B, 3, nz, ny, nx)
    field.copy_(_normal(field.shape, seed, dtype, "cuda"))
    return buf, field, field.data_ptr() + cells * field.element_size(), 3 * cells


def _lib_of(dtype):
    return L.load_f64() if dtype == torch.float64 else L.load()


def _raw_opposition(dtype, off, B, nz, ny, nx, rows, gain, actor, seed=5):
    buf, field, ptr, stride = _component_view(B, nz, ny, nx, dtype, off, seed)
    az = actor if nz > 1 else 1
    out = torch.full((B, len(rows), nx // actor, nz // az), float("nan"), dtype=dtype, device="cuda")
    lib = _lib_of(dtype)
    L.check(lib.fg_baseline_opposition(ctypes.c_void_p(ptr), stride, B, nz, ny, nx, (ctypes.c_int32 * len(rows))(*rows),
                                       (ctypes.c_double * len(gain))(*gain), len(rows), actor, ctypes.c_void_p(out.data_ptr()),
                                       ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), lib=lib)
    torch.cuda.synchronize()
    return field[:, 1].cpu().numpy(), out.cpu()


# (nz, ny, nx, actor): strips of 1, 2 and 4 patches, patches of one and of several 16-byte words, an edge that fits no word, an nx that is
# no multiple of the word, a 2-D plane, more strips than threads
OPPOSITION_SHAPES = [(8, 4, 16, 1), (8, 4, 16, 2), (8, 4, 16, 4), (16, 3, 40, 8), (6, 5, 12, 3), (6, 3, 6, 2), (1, 4, 16, 2), (64, 2, 64, 2)]


@pytest.mark.parametrize("shape", OPPOSITION_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", DTYPES.values(), ids=DTYPES.keys())
def test_opposition_kernel_forms(dtype, shape):
    nz, ny, nx, actor = shape
    rows, gain = [1, ny - 1], [-1.0, 0.5]
    v, aligned = _raw_opposition(dtype, 0, 2, nz, ny, nx, rows, gain, actor)
    v1, shifted = _raw_opposition(dtype, 1, 2, nz, ny, nx, rows, gain, actor)
    assert np.array_equal(v, v1)
    assert torch.equal(aligned, shifted)                                # 16-byte loads and single reals: the same bits
    want = R.opposition_action(v, rows, gain, actor)
    err, bound = np.abs(aligned.double().numpy() - want).max(), _bound(dtype, np.abs(v).max(), 4096)
    print(f"opposition kernel {shape}: max |error| {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    _, single = _raw_opposition(dtype, 0, 2, nz, ny, nx, rows[:1], gain[:1], actor)
    assert torch.equal(single[:, 0], aligned[:, 0])                     # a wall's action does not depend on the other wall


def _raw_pd(dtype, off, B, nz, ny, nx, seg, kp, kdt, seeds, reset_env=None):
    """One call per seed on the same buffers; ``reset_env`` gets its ``first`` flag back before the last call."""
    cells = nz * ny * nx
    buf, field, ptr, stride = _component_view(B, nz, ny, nx, dtype, off, seeds[0])
    nhz, nhx = (nz // seg if nz > 1 else 1), nx // seg
    wy = np.random.default_rng(0).uniform(0.5, 1.5, ny)
    wy /= wy.sum()
    d_wy = torch.as_tensor(wy, device="cuda")
    e_state = torch.full((B, nhz, nhx), float("nan"), dtype=torch.float64, device="cuda")
    first, tickets = torch.ones(B, dtype=torch.int32, device="cuda"), torch.zeros(B, dtype=torch.int64, device="cuda")
    lib, p = _lib_of(dtype), lambda t: ctypes.c_void_p(t.data_ptr())
    fields, outs = [], []
    for k, seed in enumerate(seeds):
        field.copy_(_normal(field.shape, seed, dtype, "cuda"))
        if reset_env is not None and k == len(seeds) - 1:
            first[reset_env] = 1
        out = torch.full((B, nhz, nhx), float("nan"), dtype=dtype, device="cuda")
        L.check(lib.fg_baseline_pd(ctypes.c_void_p(ptr), stride, B, nz, ny, nx, seg, p(d_wy), kp, kdt, p(e_state), p(first), p(tickets), p(out),
                                   ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), lib=lib)
        torch.cuda.synchronize()
        assert first.tolist() == [0] * B and tickets.tolist() == [(k + 1) * nhz * nhx] * B
        fields.append(field[:, 1].cpu().numpy())
        outs.append(out.cpu())
    return wy, fields, outs


# (nz, ny, nx, seg): a wave per heater and a workgroup per heater (columns of more than 1024 cells), 2-D and 3-D, a seg that fits no word
PD_SHAPES = [(1, 20, 32, 8), (1, 7, 12, 3), (1, 300, 8, 4), (8, 5, 8, 4), (16, 17, 16, 8), (6, 9, 6, 2)]


@pytest.mark.parametrize("shape", PD_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", DTYPES.values(), ids=DTYPES.keys())
def test_pd_kernel_forms(dtype, shape):
    nz, ny, nx, seg = shape
    kp, kdt, seeds = 970.0, 2000.0, [1, 2, 3]
    wy, fields, aligned = _raw_pd(dtype, 0, 3, nz, ny, nx, seg, kp, kdt, seeds, reset_env=1)
    _, _, shifted = _raw_pd(dtype, 1, 3, nz, ny, nx, seg, kp, kdt, seeds, reset_env=1)
    ref = R.PDController(3, kp, kdt)
    cells = (seg if nz > 1 else 1) * ny * seg
    bound = _bound(dtype, max(np.abs(f).max() for f in fields), cells, kp + 2 * kdt)
    for k, (f, a, s) in enumerate(zip(fields, aligned, shifted)):
        assert torch.equal(a, s)                                        # 16-byte loads and single reals: the same bits
        if k == 2:
            ref.reset([1])
        err = np.abs(a.double().numpy() - ref.action(f, wy, seg)).max()
        print(f"pd kernel {shape} call {k}: max |error| {err:.3e}, bound {bound:.3e}")
        assert err <= bound
    E = R.pd_energy(fields[2], wy, seg)
    assert np.abs(aligned[2][1].double().numpy() + kp * E[1]).max() <= bound          # env 1: no derivative after its reset
    assert np.abs(aligned[2][0].double().numpy() + kp * E[0]).max() > 100 * bound     # env 0 kept it


# ------------------------------------------------------------------------------------------------ opposition control on the envs
TCF_SHAPES = {
    "24x16-actor2": dict(resolution_x=24, resolution_z=16, actor_size=2),      # X != Z, rows no multiple of 64, 96 patches < 256 threads
    "32x16-actor4": dict(resolution_x=32, resolution_z=16, actor_size=4),
    "64x64-actor2": dict(resolution_x_z=64, actor_size=2),                     # 1024 patches: more than one per thread
}


@pytest.mark.parametrize("shape", TCF_SHAPES.keys())
@pytest.mark.parametrize("dtype", DTYPES.values(), ids=DTYPES.keys())
@pytest.mark.parametrize("use_marl", [False, True], ids=["sarl", "marl"])
@pytest.mark.parametrize("env_id", ["TCFSmall3D-both-easy-v0", "TCFSmall3D-bottom-easy-v0"])
def test_opposition_control_against_the_restatement(env_id, use_marl, dtype, shape):
    env = fluidgym_amd.make(env_id, num_envs=2, resolution_y=16, use_marl=use_marl, dtype=dtype, randomize_initial_state=False,
                            **TCF_SHAPES[shape])
    try:
        env.reset(seed=3)
        env.scale_actions = False
        ctrl = OppositionControl(env)
        W, actor = ctrl.n_walls, env._actor_size
        assert W == (2 if "both" in env_id else 1)
        rows = ctrl.detection_rows()
        assert rows == [env._y_obs_bottom_idx, 16 - 1 - env._y_obs_bottom_idx][:W]      # the true mirror, not the observation's ny - idx
        u = env._block.velocity
        field = _normal(u.shape, 11, dtype, u.device)
        env._block.setVelocity(field)
        a = ctrl.action()
        assert a.shape == env.sample_action().shape and a.dtype == dtype
        v = env._block.velocity[:, 1].cpu().numpy()
        want = R.opposition_action(v, rows, [-1.0, 1.0][:W], actor)
        got = a.double().cpu().numpy().reshape(want.shape)
        bound = _bound(dtype, np.abs(v).max(), 4096)
        err, net = np.abs(got - want).max(), np.abs(got.sum(axis=(2, 3))).max()
        n_patches = want.shape[2] * want.shape[3]
        print(f"{env_id} {shape}: max |error| {err:.3e} (bound {bound:.3e}), max |sum over a wall| {net:.3e} (bound {n_patches * bound:.3e})")
        assert err <= bound
        assert net <= n_patches * bound
        # identical envs: identical bits; the same batch again: the same bits
        field[1] = field[0]
        env._block.setVelocity(field)
        twin = ctrl.action()
        assert torch.equal(twin[0], twin[1])
        assert torch.equal(ctrl.action(), twin)
    finally:
        env.close()


def test_opposition_action_through_the_env_lands_on_the_walls():
    env = fluidgym_amd.make("TCFSmall3D-both-easy-v0", num_envs=2, resolution_y=16, resolution_x_z=16, actor_size=2, use_marl=False,
                            randomize_initial_state=False)
    try:
        env.reset(seed=4)
        ctrl = OppositionControl(env)
        assert env.scale_actions
        with pytest.raises(RuntimeError, match="scale_actions"):
            ctrl.action()
        env.scale_actions = False
        a = ctrl.action().clone()
        assert float(a.abs().max()) > 0.0
        env.step(a)
        rep = a.reshape(2, 2, 8, 8).repeat_interleave(2, dim=2).repeat_interleave(2, dim=3).transpose(2, 3)      # [B, wall, Z, X]
        lo, hi = env._bottom_plate.velocity, env._top_plate.velocity                                             # [B, 3, Z, 1, X]
        assert torch.equal(lo[:, 1, :, 0, :], rep[:, 0]) and torch.equal(hi[:, 1, :, 0, :], -rep[:, 1])
        for plate in (lo, hi):
            assert not plate[:, 0].any() and not plate[:, 2].any()
    finally:
        env.close()


# ------------------------------------------------------------------------------------------------ PD control on the envs
RBC_CASES = {
    "RBC2D": ("RBC2D-easy-v0", dict(num_envs=3, n_heaters=4, resolution=8)),
    "RBC3D": ("RBC3D-easy-v0", dict(num_envs=3, n_heaters=2, resolution=4, local_obs_window=1)),
}


@pytest.mark.parametrize("dtype", DTYPES.values(), ids=DTYPES.keys())
@pytest.mark.parametrize("case", RBC_CASES.keys())
def test_pd_control_against_the_restatement(case, dtype):
    env_id, kw = RBC_CASES[case]
    env = fluidgym_amd.make(env_id, dtype=dtype, randomize_initial_state=False, **kw)
    try:
        env.reset(seed=1)
        blk, seg = env._block, env._heater_width
        u = blk.velocity
        h = np.diff(np.asarray(blk.edges[1], np.float64))
        wy = h / h.sum()
        kdt = 2000.0 / env.step_length
        ctrl, twin, ref = PDControl(env), PDControl(env), R.PDController(3, 970.0, kdt)
        v_of = lambda: blk.velocity[:, 1].reshape(3, -1, *u.shape[-2:]).cpu().numpy()                        # [B, nz, ny, nx]
        cells = (seg if env.ndims == 3 else 1) * u.shape[-2] * seg

        def call(seed, what):
            blk.setVelocity(_normal(u.shape, seed, dtype, u.device, 0.05))
            a, b = ctrl.action(), twin.action()
            assert torch.equal(a, b) and a.shape == env.sample_action().shape and a.dtype == dtype
            v = v_of()
            want = ref.action(v, wy, seg)
            bound = _bound(dtype, np.abs(v).max(), cells, 970.0 + 2 * kdt)
            err = np.abs(a.double().cpu().numpy().reshape(want.shape) - want).max()
            print(f"{case} {what}: max |error| {err:.3e}, bound {bound:.3e}")
            assert err <= bound
            return a.double().cpu().numpy().reshape(want.shape), R.pd_energy(v, wy, seg), bound

        call(21, "first call")
        a2, E2, bound = call(22, "second call")
        assert np.abs(a2 + 970.0 * E2).max() > 100 * bound                     # the stored E is in use
        ctrl.reset(envs=[1]), twin.reset(envs=[1]), ref.reset([1])
        a3, E3, bound = call(23, "after reset(envs=[1])")
        assert np.abs(a3[1] + 970.0 * E3[1]).max() <= bound                    # env 1 alone lost its derivative
        assert np.abs(a3[[0, 2]] + 970.0 * E3[[0, 2]]).max() > 100 * bound
        # reset_envs([1]) + reset([1]): the other envs' actions keep their bits
        blk.setVelocity(_normal(u.shape, 24, dtype, u.device, 0.05))
        keep = ctrl.action()
        env.reset_envs([1])
        twin.reset([1])
        after = twin.action()
        assert torch.equal(after[[0, 2]], keep[[0, 2]])
        E = R.pd_energy(v_of(), wy, seg)
        assert np.abs(after[1].double().cpu().numpy().reshape(E[1].shape) + 970.0 * E[1]).max() <= bound
    finally:
        env.close()


# ------------------------------------------------------------------------------------------------ episodes
@pytest.fixture
def data_path(tmp_path, monkeypatch):
    monkeypatch.setenv("FLUIDGYM_DATA_PATH", str(tmp_path))
    monkeypatch.setitem(fluidgym_amd.config.settings, "local_data_path", None)
    return tmp_path


def test_opposition_control_episodes_and_their_files(data_path):
    env = fluidgym_amd.make("TCFSmall3D-both-easy-v0", num_envs=2, resolution_y=16, resolution_x_z=16, randomize_initial_state=False)
    try:
        frames = run_baseline_episodes(env, OppositionControl(env), seed=5, steps=3)
        assert env.scale_actions                                               # put back
        assert len(frames) == 2
        for df in frames:
            assert list(df.columns[:2]) == ["step", "reward"]
            assert set(df.columns[2:]) == {"wall_stress", "wall_stress_bottom", "wall_stress_top", "global_reward"}
            assert len(df) == 3 and df["step"].tolist() == [0, 1, 2]
            assert np.isfinite(df.to_numpy(dtype=np.float64)).all()
        env._get_domain_dir(0).mkdir(parents=True)
        env.save_opposition_control_episode(0, EnvMode.TRAIN, frames[1])
        back = env.load_opposition_control_episode(0, EnvMode.TRAIN)
        assert list(back.columns) == list(frames[1].columns)
        assert np.allclose(back.to_numpy(dtype=np.float64), frames[1].to_numpy(dtype=np.float64), rtol=1e-12, atol=0.0)
    finally:
        env.close()


def test_pd_control_episodes():
    env = fluidgym_amd.make("RBC2D-easy-v0", num_envs=2, n_heaters=4, resolution=8, randomize_initial_state=False, step_length=0.2)
    try:
        frames = run_baseline_episodes(env, PDControl(env), seed=5, steps=2)
        assert len(frames) == 2
        for df in frames:
            assert list(df.columns) == ["step", "reward", "nusselt"] and len(df) == 2
            assert np.isfinite(df.to_numpy(dtype=np.float64)).all()
    finally:
        env.close()
