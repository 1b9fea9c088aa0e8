"""``start_flow_spectra`` / ``stop_flow_spectra`` of the TCF and RBC envs: the sample an env step takes is the spectrum of the
block's fields, the moments recorded alongside keep their bits, recording leaves the simulation untouched, and the envs whose grids
the kernel does not take say so.

The TCF env runs at 16 x 16 x 16, the grid of ``test_gpu_flow_statistics.py``: x and z are supported powers of two."""
import functools

import numpy as np
import pytest
import torch

import fluidgym_amd
from fluidgym_amd.simulation.plane_spectra import HostPlaneSpectra, PlaneSpectra
from tests.plane_spectra_ref import bound_ratios, direct_sums

pytestmark = pytest.mark.gpu

TCF = dict(num_envs=2, randomize_initial_state=False, resolution_x_z=16, resolution_y=16, step_length=0.6, use_marl=False)
PLANES = (5, 1)


@functools.lru_cache(maxsize=None)
def _tcf_run(moments: bool, spectra: bool):
    """One env step from the same start; what was recorded and the state it left."""
    env = fluidgym_amd.make("TCFSmall3D-both-easy-v0", **TCF)
    env.reset(seed=4)
    assert env._hook("flow_spectra") is None and env._hook("flow_stats") is None
    if moments:
        env.start_flow_statistics(order=2)
    if spectra:
        env.start_flow_spectra(PLANES, every=env._n_sim_steps)
    a = (torch.rand(env._zero_action.shape, generator=torch.Generator().manual_seed(0)) * 2 - 1).to(env.cuda_device)
    env.step(a)
    out = {"velocity": env._block.velocity.clone(), "pressure": env._block.pressure.clone(), "sim_steps": env._n_sim_steps}
    if moments:
        out["moments"] = env.stop_flow_statistics()
    if spectra:
        out["spectra"] = env.stop_flow_spectra()
        assert env._hook("flow_spectra") is None
        with pytest.raises(RuntimeError, match="no spectra"):
            env.stop_flow_spectra()
    env.close()
    return out


def test_one_env_step_takes_the_spectrum_of_the_blocks_fields():
    run = _tcf_run(True, True)
    rec = run["spectra"]
    assert isinstance(rec, PlaneSpectra) and rec.channels == ("u", "v", "w", "p") and rec.planes == PLANES and rec.symmetric
    assert rec.samples == 1 and rec.n == 2 * 2
    u, p = run["velocity"].cpu().numpy(), run["pressure"].cpu().numpy()
    host = HostPlaneSpectra(rec.channels, PLANES, True)
    host.update(u, p)
    stack = np.concatenate([np.moveaxis(u, 1, 0), np.moveaxis(p, 1, 0)]).astype(np.float64)          # [K, B, nz, ny, nx]
    truth = direct_sums([stack], rec.plane_table(16))
    _, amp, power = rec._state()
    ra, rp = bound_ratios(amp, power, truth, float(np.finfo(np.float32).eps), 16, 16)
    ha, hp = bound_ratios(amp, power, host._state()[1:] + truth[2:], float(np.finfo(np.float32).eps), 16, 16)
    print(f"TCF 16^3 sample: error / bound against numpy amp {ra:.3g} power {rp:.3g}; against the host twin amp {ha:.3g} power {hp:.3g}")
    assert max(ra, rp, ha, hp) <= 1
    assert rec.amplitude("u").shape == (2, 2, 8, 8) and np.all(rec.amplitude("u")[:, :, 0, 0] > 0)     # the mean flow sits in mode (0, 0)
    lam, phi = rec.pooled().premultiplied("u", [np.pi, 2 * np.pi], 1e-3, 0.05)
    assert phi.shape == (1, 2, 8, 8) and lam[0].shape == lam[1].shape == (8,)


def test_the_moments_alongside_keep_their_bits_and_the_state_is_left_alone():
    alone, both, off = _tcf_run(True, False), _tcf_run(True, True), _tcf_run(False, False)
    for a, b in zip(alone["moments"]._state(), both["moments"]._state()):
        assert a.tobytes() == b.tobytes()
    for run in (alone, both):
        assert torch.equal(run["velocity"], off["velocity"]) and torch.equal(run["pressure"], off["pressure"])


def test_spectra_need_a_reset_a_valid_period_and_planes_of_the_grid():
    env = fluidgym_amd.make("TCFSmall3D-both-easy-v0", **TCF)
    with pytest.raises(RuntimeError, match="reset"):
        env.start_flow_spectra((1,))
    with pytest.raises(RuntimeError, match="no spectra"):
        env.stop_flow_spectra()
    env.reset(seed=4)
    with pytest.raises(ValueError, match="every"):
        env.start_flow_spectra((1,), every=0)
    with pytest.raises(ValueError, match="outside the 16 rows"):
        env.start_flow_spectra((16,))
    assert env._hook("flow_spectra") is None
    env.start_flow_spectra((1,), every=2, symmetric=False)
    env.step(torch.zeros(env._zero_action.shape, device=env.cuda_device))
    rec = env.stop_flow_spectra()
    assert rec.samples == env._n_sim_steps // 2 and rec.n == 2 * rec.samples and rec.amplitude("w").shape == (2, 1, 8, 8)
    env.close()


def test_rbc2d_takes_the_spectrum_along_x_where_nx_is_a_power_of_two():
    env = fluidgym_amd.make("RBC2D-easy-v0", num_envs=2, n_heaters=3, resolution=8, randomize_initial_state=False, step_length=0.5)
    env.reset(seed=1)
    assert env._block.velocity.shape[-1] == 24
    with pytest.raises(ValueError, match="nx must be a power of two"):
        env.start_flow_spectra((1,))
    assert env._hook("flow_spectra") is None
    env.close()
    env = fluidgym_amd.make("RBC2D-easy-v0", num_envs=2, n_heaters=4, resolution=8, randomize_initial_state=False, step_length=0.5)
    env.reset(seed=1)
    env.start_flow_spectra((2,))
    env.step(torch.zeros(2, 4, 1, device="cuda"))
    rec = env.stop_flow_spectra()
    assert rec.channels == ("u", "v", "p", "T") and rec.samples == env._n_sim_steps and rec.n == 2 * 2 * rec.samples
    T = rec.amplitude("T")
    print("temperature spectrum of env 0, row 2:", T[0, 0, 0])
    assert T.shape == (2, 1, 1, 16) and np.isfinite(T).all() and np.all(T[:, :, 0, 0] > 0)
    env.close()


def test_a_multi_block_env_refuses():
    env = fluidgym_amd.make("CylinderJet2D-easy-v0", num_envs=1, initial_domain_steps=1, randomize_initial_state=False)
    env.reset(seed=0)
    with pytest.raises(NotImplementedError, match="single-block"):
        env.start_flow_spectra((1,))
    with pytest.raises(NotImplementedError, match="single-block"):
        env.start_flow_statistics()
    env.close()
