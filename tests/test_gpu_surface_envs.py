"""``get_surface_distribution`` and ``start_field_statistics(surface=True)`` on the smallest cylinder and airfoil envs: the curves
integrate to the env's own wall forces and coefficients, ``p_ref`` moves ``cp`` only, the coordinates follow the ring, the recorded
sample is the curve of the step it was taken after, identical envs record identical bits, and the envs without a ring refuse."""
import numpy as np
import pytest
import torch

import fluidgym_amd

pytestmark = pytest.mark.gpu

ENVS = {
    "CylinderJet2D-easy-v0": dict(num_envs=2, resolution=8, initial_domain_steps=3, randomize_initial_state=False),
    "CylinderJet3D-easy-v0": dict(num_envs=2, resolution=8, initial_domain_steps=3, randomize_initial_state=False),
    "Airfoil2D-easy-v0": dict(num_envs=2, resolution_div=2, initial_domain_steps=6, randomize_initial_state=False, episode_length=3),
}
FORCE_TOL = 2e-5        # x the largest force: the figure of test_wall_force_kernel_is_the_tensor_form (another summation order)


def _opposite_actions(env):
    act = torch.full_like(env._zero_action, 0.5)
    act[1] = -0.5
    return act


@pytest.fixture(scope="module", params=list(ENVS))
def stepped(request):
    """The env after a few initial-domain steps and one env step with opposite actions in its two envs."""
    env = fluidgym_amd.make(request.param, **ENVS[request.param])
    env.reset(seed=0)
    env.step(_opposite_actions(env))
    yield request.param, env
    env.close()


def test_curves_integrate_to_the_wall_forces_and_coefficients(stepped):
    env_id, env = stepped
    dom, ring = env._domain, env._ring
    saved = dom.Clone()
    g = torch.Generator(device="cpu").manual_seed(3)
    dom.velocity.add_((0.2 * torch.randn(dom.velocity.shape, generator=g)).cuda())       # a field with real wall gradients
    dom.pressure.add_((0.5 * torch.randn(dom.pressure.shape, generator=g)).cuda())
    nu, lh = env._wall_force_args()
    sd = env.get_surface_distribution()
    n, nz = ring.n_faces, ring.nz
    shape = (2, n) if env._ndims == 2 else (2, nz, n)
    assert tuple(sd.p.shape) == tuple(sd.tau_w.shape) == tuple(sd.cp.shape) == tuple(sd.cf.shape) == shape
    assert tuple(sd.traction.shape) == (2, 2) + shape[1:] and sd.p.is_cuda and sd.p.dtype == dom.dtype
    want = ring.forces(dom, nu, layer_height=lh)
    got = sd.forces(lh)
    scale = want.abs().max().item()
    assert got.shape == want.shape and scale > 1e-3
    print(f"{env_id}: forces differ by {(got - want).abs().max().item() / scale:.2e} of the largest")
    assert (got - want).abs().max().item() <= FORCE_TOL * scale
    assert torch.equal(sd.forces(), got)                      # the env's own layer height is the default
    cd, cl = env._get_drag_and_lift()
    norm = sd.q * (env.airfoil_length if "Airfoil" in env_id else env.cylinder_diameter)       # as _get_drag_and_lift divides
    gd, gl = got[:, 0] / norm, got[:, 1] / norm
    cscale = max(cd.abs().max().item(), cl.abs().max().item())
    assert gd.shape == cd.shape and (gd - cd).abs().max().item() <= FORCE_TOL * cscale and (gl - cl).abs().max().item() <= FORCE_TOL * cscale
    # the curve is the ring's distribution, and cf its shear over q
    d = ring.distribution(dom, nu)
    assert tuple(d.shape) == (2, 4, nz, n)
    assert torch.equal(d[:, 1].reshape(shape), sd.tau_w) and torch.equal(sd.cf, sd.tau_w / sd.q) and sd.q == 0.5 * env._U_mean ** 2
    assert sd.tau_w.abs().max().item() > 0
    dom.Restore(saved)


def test_p_ref_moves_cp_only_and_the_coordinates_follow_the_ring(stepped):
    env_id, env = stepped
    n = env._ring.n_faces
    a = env.get_surface_distribution()
    b = env.get_surface_distribution(p_ref=0.25)
    c = env.get_surface_distribution(p_ref=torch.tensor([0.25, -1.0]))
    for x in (b, c):
        assert torch.equal(x.p, a.p) and torch.equal(x.tau_w, a.tau_w) and torch.equal(x.traction, a.traction) and torch.equal(x.cf, a.cf)
    assert torch.equal(a.cp, a.p / a.q) and torch.equal(b.cp, (a.p - 0.25) / a.q)
    assert torch.equal(c.cp[0], b.cp[0]) and torch.equal(c.cp[1], (a.p[1] + 1.0) / a.q)
    with pytest.raises(ValueError, match="p_ref"):
        env.get_surface_distribution(p_ref=torch.zeros(3))
    assert tuple(a.arc_length.shape) == (n,) and tuple(a.face_centers.shape) == (2, n) and tuple(a.face_lengths.shape) == (n,)
    assert bool((a.arc_length[1:] > a.arc_length[:-1]).all()) and a.arc_length[-1].item() < a.perimeter
    if "Airfoil" in env_id:
        assert a.theta is None and tuple(a.x_over_c.shape) == tuple(a.side.shape) == (n,)
        assert 0.0 < a.x_over_c.min().item() and a.x_over_c.max().item() < 1.0 and set(a.side.tolist()) == {1.0, -1.0}
    else:
        assert a.x_over_c is None and a.side is None and tuple(a.theta.shape) == (n,)
        assert -180.0 < a.theta.min().item() and a.theta.max().item() <= 180.0
    pts = a.separation_points()
    assert len(pts) == 2 and all(isinstance(s, np.ndarray) and np.all((s >= 0) & (s < a.perimeter)) for s in pts)
    assert all(len(s) % 2 == 0 for s in pts)                  # a closed curve changes sign an even number of times


def test_surface_statistics_ride_on_the_field_statistics_hook(stepped):
    env_id, env = stepped
    env.start_field_statistics(every=env._n_sim_steps)
    env.step(_opposite_actions(env))
    assert env.stop_field_statistics().surface is None        # the default: as before
    env.start_field_statistics(every=env._n_sim_steps, surface=True)
    env.step(_opposite_actions(env))
    rec = env.stop_field_statistics()
    wall = rec.surface
    assert rec.samples == 1 and wall.samples == 1 and wall.n_faces == env._ring.n_faces and wall.layers == env._ring.nz
    sd = env.get_surface_distribution()
    curves = {"p": sd.p, "tau_w": sd.tau_w, "fx": sd.traction[:, 0], "fy": sd.traction[:, 1]}
    for ch, t in curves.items():
        got, want = wall.mean(ch), t.double().cpu().numpy()
        if env._ndims == 2:
            assert got.tobytes() == want.tobytes(), ch      # the sample after the step's last sim step is the curve of the state
            assert not wall.variance(ch).any()
        else:                                                 # span-averaged: the fp64 mean over the layers, in the kernel's order
            assert got.shape == (2, env._ring.n_faces)
            acc = np.zeros_like(got)
            for z in range(want.shape[1]):
                acc = acc + want[:, z]
            assert np.array_equal(got, acc / want.shape[1]), ch
    with pytest.raises(RuntimeError):
        env.stop_field_statistics()


def test_two_identical_envs_record_identical_bits():
    kw = dict(ENVS["CylinderJet2D-easy-v0"])
    env = fluidgym_amd.make("CylinderJet2D-easy-v0", **kw)
    env.reset(seed=0)
    env.start_field_statistics(every=1, surface=True)
    for _ in range(2):
        env.step(torch.full_like(env._zero_action, 0.5))
    wall = env.stop_field_statistics().surface
    mean, cen = wall._state()
    assert wall.samples == 2 * env._n_sim_steps
    assert mean[0].tobytes() == mean[1].tobytes() and cen[0].tobytes() == cen[1].tobytes()
    assert wall.variance("tau_w").max() > 0 and wall.pooled().samples == 2 * wall.samples
    env.close()


def test_envs_without_a_wall_ring_refuse():
    from fluidgym_amd.envs.parallel_env import ParallelFluidEnv

    env = fluidgym_amd.make("RBC2D-easy-v0")
    with pytest.raises(NotImplementedError, match="wall ring"):
        env.get_surface_distribution()
    env.close()
    with pytest.raises(NotImplementedError, match="ParallelFluidEnv"):
        ParallelFluidEnv.get_surface_distribution(None)
    fresh = fluidgym_amd.make("CylinderJet2D-easy-v0", **ENVS["CylinderJet2D-easy-v0"])
    with pytest.raises(RuntimeError, match="reset"):
        fresh.get_surface_distribution()
    fresh.close()
