"""What ``envs/mesh_body.py`` holds for the cylinder and the airfoil envs, on the host (construction touches no GPU): the smoothing
recurrence of the env step, the spanwise observation layout on the airfoil, the draw of the randomisation warm-up and the force hooks."""
import numpy as np
import pytest
import torch

import fluidgym_amd
from fluidgym_amd.envs.mesh_body import MeshBodyEnvBase, smoothed_controls

CPU = torch.device("cpu")


@pytest.mark.parametrize("state_dtype", [torch.float32, torch.float64])
def test_smoothed_controls_is_the_per_step_tensor_expression(state_dtype):
    """``c = c + alpha * (t - c)`` step by step, bit for bit; an fp32 target against an fp64 state covers the promotion."""
    g = torch.Generator().manual_seed(5)
    B, n_controls, n, alpha = 3, 12, 5, 0.1
    start = torch.randn(B, n_controls, generator=g).to(state_dtype)
    target = torch.rand(B, n_controls, generator=g) * 2 - 1                # fp32
    assert float(start.abs().min()) > 0
    got = smoothed_controls(start, target, alpha, n)
    assert got.shape == (n, B, n_controls) and got.dtype == state_dtype
    c = start
    for k in range(n):
        c = c + alpha * (target - c)
        assert torch.equal(got[k], c), k
    assert not torch.equal(got[0], got[n - 1])


def _expected_airfoil_obs(env, window):
    """The reference's definition (obs_extraction.py, ``extract_global_3d_obs`` / ``transform_global_to_local_obs_3d``), written out:
    gather as [z, sensor, component], reinterpret the memory as [z, component, sensor], split z into agents x sensors per agent;
    agent a sees the agents a - W//2 ... a + W//2, periodically."""
    rs, px = env.render_shape, env._sensor_locations                       # px [3, nz, n]
    nz, n = px.shape[1], px.shape[2]
    flat = px[0] + rs[0] * (px[1] + rs[1] * px[2])                          # [nz, n]: the pixel of every sensor in the flat fields
    comps = 2 if env._local_2d_obs else 3
    u, p = env._domain.velocity[0].numpy(), env._domain.pressure[0].numpy()
    gathered = np.stack([u[c][flat] for c in range(comps)], axis=-1)       # [z, sensor, component]
    vel = np.ascontiguousarray(gathered).reshape(nz, comps, n)             # the view
    na, spa = env._n_agents, env._n_sensors_per_agent
    vel = vel.reshape(na, spa, comps, n)
    if env._local_2d_obs:
        vel = vel.transpose(0, 1, 3, 2)
    pres = p[flat].reshape(na, spa, n)
    if window is None:
        return vel, pres
    idx = [[(a - window // 2 + k) % na for k in range(window)] for a in range(na)]
    lv, lp = vel[np.asarray(idx)], pres[np.asarray(idx)]                    # [agent, window, spa, ...]
    if env._local_2d_obs:
        lv, lp = lv[:, 0, 0], lp[:, 0, 0]
    return lv, lp


@pytest.mark.parametrize("use_marl,window,local_2d", [(False, 1, False), (True, 1, False), (True, 3, False), (True, 1, True)])
def test_airfoil_3d_observation_layout_and_local_windows(use_marl, window, local_2d):
    from tests.helpers_mb import ramp_obs_env

    env = ramp_obs_env("Airfoil3D-easy-v0", res_z=8, n_agents=4, resolution_div=4, use_marl=use_marl, local_obs_window=window,
                       local_2d_obs=local_2d)
    gv, gp = _expected_airfoil_obs(env, None)
    obs = env._get_global_obs()
    assert np.array_equal(obs["velocity"][0].numpy(), gv) and np.array_equal(obs["pressure"][0].numpy(), gp)
    if not use_marl:
        assert tuple(obs["velocity"].shape[1:]) == env.observation_space["velocity"].shape
        return
    lv, lp = _expected_airfoil_obs(env, window)
    local = env._get_local_obs()
    assert np.array_equal(local["velocity"][0].numpy(), lv) and np.array_equal(local["pressure"][0].numpy(), lp)
    assert tuple(local["velocity"].shape[2:]) == env.observation_space["velocity"].shape
    assert tuple(local["pressure"].shape[2:]) == env.observation_space["pressure"].shape
    assert len(np.unique(lp)) > 1


@pytest.mark.parametrize("env_id", ["CylinderJet2D-easy-v0", "Airfoil2D-easy-v0", "Airfoil3D-easy-v0"])
def test_randomize_n_steps_is_the_reference_draw(env_id):
    """cylinder_env_base.py:364-372: ``max_n`` = two shedding periods in env steps less one; airfoil_env_base.py:327-329: 5 % of the
    episode; the count is ``integers(int(0.5 max_n), max_n) + 1``, one draw from the env's NumPy generator."""
    env = fluidgym_amd.make(env_id, cuda_device=CPU)
    if "Cylinder" in env_id:
        period = 1.0 / (0.3 * 1.0 / 1.0)
        max_n = 2 * int(period / env.step_length) - 1
    else:
        max_n = int(0.05 * env.episode_length)
    assert max_n > 2
    for seed in (0, 7):
        env._np_rng, ref = np.random.default_rng(seed), np.random.default_rng(seed)
        want = int(ref.integers(int(0.5 * max_n), max_n)) + 1
        assert env._randomize_n_steps() == want
        assert env._np_rng.integers(0, 1 << 30) == ref.integers(0, 1 << 30)      # exactly one draw was consumed


@pytest.mark.parametrize("env_id,kw,layer_height,force_norm", [
    ("CylinderJet2D-easy-v0", {}, 4.0 / 24, 0.5 * 1.0 ** 2 * 1.0),
    ("CylinderRot2D-easy-v0", {"resolution": 8}, 4.0 / 8, 0.5 * 1.0 ** 2 * 1.0),
    ("CylinderJet3D-easy-v0", {"resolution": 8, "n_jets": 4}, 4.0 / 8, 0.5 * 1.0 ** 2 * 1.0),
    ("Airfoil2D-easy-v0", {}, 1.0, 0.5 * 0.3 ** 2 * 1.0),              # 2-D: no spanwise layer, the wall-force launch takes 1
    ("Airfoil3D-easy-v0", {"res_z": 8}, 1.4 / 8, 0.5 * 0.3 ** 2 * 1.0),
])
def test_layer_height_and_force_norm(env_id, kw, layer_height, force_norm):
    """D / resolution (cylinder), D / res_z (3-D airfoil) and 0.5 U^2 L, from the constants of the reference's classes."""
    env = fluidgym_amd.make(env_id, cuda_device=CPU, **kw)
    assert isinstance(env, MeshBodyEnvBase)
    assert env._layer_height == layer_height and env._force_norm == force_norm
    cls = type(env)
    length = cls.cylinder_diameter if "Cylinder" in env_id else cls.airfoil_length
    assert env._force_norm == 0.5 * cls._U_mean ** 2 * length
    if env_id != "Airfoil2D-easy-v0":
        assert env._layer_height == cls.D / (env._res_z if "Airfoil" in env_id else env._circle_resolution_angular)


def test_airfoil_is_no_cylinder():
    from fluidgym_amd.envs.airfoil import AirfoilEnvBase

    assert not any(c.__name__.startswith("Cylinder") for c in AirfoilEnvBase.__mro__)
    assert not hasattr(AirfoilEnvBase, "cylinder_diameter") and not hasattr(AirfoilEnvBase, "_get_cylinder_mask")
