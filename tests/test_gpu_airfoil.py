"""Airfoil environment on the multi-block HIP path (reference ids; the mesh generator is pinned on the CPU,
tests/test_airfoil_grid.py)."""
import numpy as np
import pytest
import torch

import fluidgym_amd

pytestmark = pytest.mark.gpu

KW = dict(initial_domain_steps=6, randomize_initial_state=False, episode_length=3, resolution_div=2)


def test_env_contract_and_forces():
    env = fluidgym_amd.make("Airfoil2D-easy-v0", num_envs=2, **KW)
    obs, _ = env.reset(seed=0)
    n = env._sensor_locations.shape[1]
    assert obs["velocity"].shape == (2, n, 2) and obs["pressure"].shape == (2, n)
    assert torch.isfinite(obs["velocity"]).all()
    for i in range(3):
        a = env.sample_action()
        assert a.shape == (2, 3)
        obs, reward, term, trunc, info = env.step(0.3 * a)   # moderate jets
        assert reward.shape == (2,) and torch.isfinite(reward).all()
        assert set(info) == {"drag", "lift"} and (info["drag"] > 0).all()
        assert term is False and trunc == (i == 2)
    # lift at 10 degrees is positive and the reward is lift / drag
    assert (info["lift"] > 0).all()
    assert torch.allclose(reward, info["lift"] / info["drag"], rtol=1e-5)
    env.close()


def test_jets_blow_along_the_wall_normal_with_zero_net_action_and_fluxes_balance():
    from fluidgym_amd.envs.airfoil_grid import TOP

    env = fluidgym_amd.make("Airfoil2D-easy-v0", num_envs=2, **KW)
    env.reset(seed=1)
    act = torch.tensor([[1.0, 0.0, -1.0], [0.7, 0.7, 0.7]], device="cuda")
    env._apply_action(act)                                   # no smoothing: the control itself
    wall = env._domain.blocks[TOP].boundary("-y")           # [B, 2, nx]
    (a0, a1), _, (c0, c1) = env._jet_locations_top
    normals = env._ring.wall_normals[:, env._mesh.coords[1].shape[1] + a0: env._mesh.coords[1].shape[1] + a1 + 1]
    blow = (wall[0, :, a0:a1 + 1] * normals).sum(0)
    suck = (wall[0, :, c0:c1 + 1] * env._ring.wall_normals[:, env._mesh.coords[1].shape[1] + c0: env._mesh.coords[1].shape[1] + c1 + 1]).sum(0)
    assert (blow > 0).all() and (suck < 0).all()
    # unit-sum profiles x (+1, -1), up to the cosine between neighbouring normals (the reference's index offset) and the
    # flux balancing that rescales the top face together with the outflows
    assert abs(float(blow.sum()) - 1.0) < 0.1 and abs(float(suck.sum()) + 1.0) < 0.1
    assert float(wall[1].abs().max()) < 1e-6               # equal actions: mean removed, nothing blows
    assert np.abs(env._domain.boundary_flux_balance()).max() < 1e-5
    # the torch-side flux weights are the native ones: same imbalance before balancing
    env._domain.blocks[TOP].boundary("-y")[0, 1, a0:a1 + 1] += 0.5
    native = env._domain.boundary_flux_balance()
    mine = (env._domain.boundary_velocity * env._flux_w[None]).sum((1, 2)).cpu().numpy()
    assert np.allclose(native, mine, rtol=1e-4, atol=1e-6) and abs(native[0]) > 1e-3
    env._balance_boundary_fluxes()
    assert np.abs(env._domain.boundary_flux_balance()).max() < 1e-5
    env.close()


def test_sensor_gather_equals_masked_resampling_and_state_roundtrip():
    env = fluidgym_amd.make("Airfoil2D-easy-v0", num_envs=1, **KW)
    obs, _ = env.reset(seed=2)
    full = env.get_velocity()[0]
    assert full.shape == (2, 150, 600)
    sx, sy = env._sensor_locations
    assert torch.allclose(obs["velocity"][0], full[:, torch.as_tensor(sy), torch.as_tensor(sx)].t(), rtol=1e-5, atol=1e-6)
    assert float(full[:, torch.as_tensor(env._airfoil_mask, device="cuda")].abs().max()) == 0.0
    a = torch.tensor([[0.5, -0.2, 0.1]], device="cuda")
    s0 = env.get_state()
    r1 = env.step(a)
    u1, p1 = env._domain.velocity.clone(), env._domain.pressure.clone()
    env.set_state(s0)
    back = env.get_state()
    assert all(torch.equal(back["domain"][k], s0["domain"][k]) for k in s0["domain"])   # the round trip itself is exact
    r2 = env.step(a)
    # get_state -> set_state -> step replays EXACTLY, as in the reference (envs/fluid_env.py:1320-1363; its dots are cuBLAS calls
    # in a fixed order, cg_solver_kernel.cu:277,317): the dot products of the Krylov solvers are accumulated order-independently
    # (FgDacc, csrc/fg_internal.h), so nothing in a step depends on how the workgroups were scheduled.  Round 2 accepted 15 % here.
    assert torch.equal(env._domain.velocity, u1) and torch.equal(env._domain.pressure, p1)
    assert torch.equal(r1[4]["drag"], r2[4]["drag"]) and torch.equal(r1[4]["lift"], r2[4]["lift"])
    assert all(torch.equal(r1[0][k], r2[0][k]) for k in r1[0]) and torch.equal(r1[1], r2[1])
    env.close()


def test_pressure_solves_reach_the_reference_tolerance_and_envs_stay_identical():
    """With the refined BiCGStab every pressure solve of a step converges to 1e-7 (CG stagnates at 2-4e-5 on this mesh); identical
    envs of a batch stay BIT-identical through 12 development steps and an env step (the reductions do not depend on the order in
    which workgroups arrive), and a second process-independent run of the same env reproduces the first bit for bit."""
    def run():
        env = fluidgym_amd.make("Airfoil2D-easy-v0", num_envs=2, **dict(KW, initial_domain_steps=12))
        env.reset(seed=3)
        obs, reward, _, _, info = env.step(torch.zeros(2, 3, device="cuda"))
        out = (env._domain.velocity.clone(), env._domain.pressure.clone(), info["drag"].clone(), info["lift"].clone(),
               max(env._sim.last_iterations), env._domain.env_status().copy())
        env.close()
        return out

    u, p, drag, lift, its, status = run()
    assert its < 1500       # cold-started (reference policy): below the refined solver's cap
    assert (status == 0).all()
    assert torch.equal(u[0], u[1]) and torch.equal(p[0], p[1])
    assert torch.equal(drag[0], drag[1]) and torch.equal(lift[0], lift[1])
    assert 0.1 < float(drag[0]) < 2.0 and 0.2 < float(lift[0]) < 2.0
    u2, p2, drag2, lift2, _, _ = run()
    assert torch.equal(u, u2) and torch.equal(p, p2) and torch.equal(drag, drag2) and torch.equal(lift, lift2)


def test_multilevel_trial_of_the_pressure_bicgstab(monkeypatch):
    """The multilevel right preconditioner of the pressure BiCGStab as a trial (policy pressure_multilevel_bicgstab,
    DESIGN.md 4b) -- the mechanism.  Normal run: attempts converge (verified on the true residual) in a fraction of the plain
    iterations.  With the attempt cap forced to 2 iterations every attempt fails: the solves must be repeated with the plain
    recurrence, the handle must back off exponentially, no env may end non-finite."""
    old_policy = fluidgym_amd.set_solver_policy(pressure_multilevel_bicgstab=True)      # (the default since round 3, policy.py)

    def run(cap=None):
        if cap is not None:
            monkeypatch.setenv("FG_MB_ML_TRY_CAP", str(cap))      # read once per handle, at fg_mb_create
        else:
            monkeypatch.delenv("FG_MB_ML_TRY_CAP", raising=False)
        env = fluidgym_amd.make("Airfoil2D-easy-v0", num_envs=2, **dict(KW, initial_domain_steps=4))
        env.reset(seed=3)
        env._domain.solver_counters(reset=True)
        obs, reward, _, _, info = env.step(torch.zeros(2, 3, device="cuda"))
        out = (env._domain.multilevel_status(), env._domain.solver_counters(), info["drag"].cpu().numpy().copy(), info["lift"].cpu().numpy().copy(),
               env._domain.env_status().copy(), max(env._sim.last_iterations))
        env.close()
        return out

    try:
        st, ctr, drag, lift, status, its = run()
        st2, ctr2, drag2, lift2, status2, its2 = run(cap=2)
    finally:
        fluidgym_amd.set_solver_policy(**old_policy)
    assert st["attempts"] >= 10 and st["failed_attempts"] <= 4 and st["backoff"] <= 64, st      # (measured: 404 attempts, none failed)
    assert (status != 2).all() and its < 1500
    assert st2["failed_attempts"] == st2["attempts"] >= 3 and st2["backoff"] >= 32, st2
    assert st2["attempts"] <= 16, st2                    # exponential back-off: a handful of attempts among the ~400 solves
    assert (status2 != 2).all() and its2 < 1500
    assert ctr["pressure0"]["mean"] < 0.6 * ctr2["pressure0"]["mean"], (ctr["pressure0"], ctr2["pressure0"])   # the trial pays
    assert np.isfinite(drag).all() and np.isfinite(drag2).all()    # (the forces of the two runs are NOT compared: policy.py)


def test_restriction_fused_with_the_vector_updates_is_the_separate_launches(monkeypatch):
    """Preconditioned pressure BiCGStab: p and s formed inside the restriction of the multilevel preconditioner
    (k_ml_restrict_p / _s, the default up to 32 systems) against k_mbb_p / _s followed by k_ml_restrict (FG_MB_ML_FUSE=0, what
    larger batches run).  Same p and s; the restricted sums and s.s are added in another grouping (four threads per aggregate, one per
    row), so the two runs agree to the solver tolerance, with the same number of attempts and nearly the same iteration counts."""
    out = {}
    for fuse in ("0", "2"):
        monkeypatch.setenv("FG_MB_ML_FUSE", fuse)        # read once per handle, at fg_mb_create
        env = fluidgym_amd.make("Airfoil2D-easy-v0", num_envs=2, **dict(KW, initial_domain_steps=4))
        env.reset(seed=3)
        env._domain.solver_counters(reset=True)
        _, _, _, _, info = env.step(torch.zeros(2, 3, device="cuda"))
        out[fuse] = (env._domain.velocity.clone(), env._domain.pressure.clone(), env._domain.solver_counters(), env._domain.multilevel_status(),
                     info["drag"].clone(), env._domain.env_status().copy())
        env.close()
    (u0, p0, c0, st0, d0, s0), (u1, p1, c1, st1, d1, s1) = out["0"], out["2"]
    assert (s0 == 0).all() and (s1 == 0).all()
    assert st0["attempts"] == st1["attempts"] > 10 and st1["failed_attempts"] <= 4, (st0, st1)
    for k in ("pressure0", "pressure1"):
        assert c1[k]["unconverged"] == 0 and abs(c1[k]["mean"] - c0[k]["mean"]) < 0.1 * c0[k]["mean"], (c0[k], c1[k])
    assert float((u1 - u0).abs().max() / u0.abs().max()) < 1e-3
    # (the smoothest modes of the pressure system are the worst resolved at a given residual: the two runs -- different rounding of
    #  the restricted sums, hence different Krylov trajectories -- differ by a smooth +0.0020 .. -0.0015 at max |p| = 0.07 while the
    #  velocities agree to 1e-3; the cylinder's CG and BiCGStab differ by far more at the reference's tolerance)
    assert float((p1 - p0).abs().max() / p0.abs().max()) < 6e-2
    assert torch.allclose(d0, d1, rtol=1e-2)      # (measured 0.4236 against 0.4221: the pressure mode above, integrated over the surface)


KW3 = dict(initial_domain_steps=4, randomize_initial_state=False, episode_length=2, resolution_div=4, res_z=8, n_agents=4)


def test_3d_env_single_and_multi_agent():
    env = fluidgym_amd.make("Airfoil3D-easy-v0", num_envs=2, **KW3)
    obs, _ = env.reset(seed=0)
    n = env._sensor_locations.shape[-1]
    assert obs["velocity"].shape == (2, 4, 1, 3, n) and obs["pressure"].shape == (2, 4, 1, n)
    # started from the 2-D development extruded over the span: still uniform along z, no spanwise velocity
    for blk in env._domain.blocks:
        u = blk.cells(env._domain.velocity)[0]
        assert float((u - u[:, :1]).abs().max()) < 5e-3 and float(u[2].abs().max()) < 5e-3
    a = env.sample_action()
    assert a.shape == (2, 4, 3)
    obs, reward, term, trunc, info = env.step(0.3 * a)
    assert reward.shape == (2,) and torch.isfinite(reward).all()
    assert set(info) == {"drag", "lift", "all_cds", "all_cls"} and info["all_cds"].shape == (2, 8)
    assert torch.allclose(info["all_cds"].sum(-1) / env.D, info["drag"], rtol=1e-5) and (info["drag"] > 0).all()
    assert torch.allclose(reward, info["lift"] / info["drag"], rtol=1e-5)
    assert np.abs(env._domain.boundary_flux_balance()).max() < 1e-5
    full = env.get_velocity()
    assert full.shape == (2, 3, 150, 150, 600)
    px = env._sensor_locations.reshape(3, -1)
    u = env._sensors(env._domain.velocity)
    assert torch.allclose(full[:, :, px[2], px[1], px[0]], u, atol=1e-5)
    env.close()

    menv = fluidgym_amd.make("Airfoil3D-easy-v0", num_envs=1, use_marl=True, local_obs_window=3, **KW3)
    obs, _ = menv.reset(seed=1)
    assert obs["velocity"].shape == (1, 4, 3, 1, 3, n)
    act = torch.zeros(1, 4, 3, device="cuda")
    act[0, 0] = torch.tensor([1.0, 0.0, -1.0])
    obs, reward, _, _, info = menv.step(act)
    assert reward.shape == (1, 4) and set(info) == {"drag", "lift", "global_reward"} and torch.isfinite(reward).all()
    # only agent 0 blows: its spanwise layers carry wall velocity, the others none
    wall = menv._domain.blocks[2].boundary("-y").reshape(1, 3, 8, -1)
    assert float(wall[0, :, :2].abs().max()) > 1e-3 and float(wall[0, :, 2:].abs().max()) < 1e-6
    menv.close()


def test_replay_across_a_retry_of_the_velocity_sweeps():
    """the velocity sweeps fail on this mesh (contraction 0.8 per sweep) and back off -- the handle skips 8, 16, ... solves
    before it tries them again, and a retry that lands in one run and not in the other changes which solver ran.  The back-off
    words travel with ``get_state`` now (``fg_mb_solver_hints``: 48 words), so a replay that crosses a retry repeats bit for bit:
    three env steps (>= 30 velocity solves) from a snapshot taken with a back-off pending."""
    # (the full-resolution mesh 40 sim steps after the impulsive start: where tests/test_gpu_jacobi.py sees the sweeps fail)
    env = fluidgym_amd.make("Airfoil2D-easy-v0", num_envs=2, initial_domain_steps=40, randomize_initial_state=False, episode_length=10)
    env.reset(seed=5)
    a = torch.tensor([[0.3, -0.1, 0.2], [0.3, -0.1, 0.2]], device="cuda")
    env.step(a)
    hints = env._domain.solver_hints().tolist()
    assert len(hints) == 48 and (any(hints[36:40]) or any(hints[40:44])), hints      # a back-off is pending
    hints[36:40] = [3] * 4                                                             # ... and is made short: the next retry is three solves away
    hints[40:44] = [1] * 4
    env._domain.solver_hints(hints)
    s0 = env.get_state()
    c0 = env._domain.advection_jacobi_counts()
    for _ in range(3):
        r1 = env.step(a)
    u1, p1 = env._domain.velocity.clone(), env._domain.pressure.clone()
    c1 = env._domain.advection_jacobi_counts()
    assert c1["handed_to_bicgstab"] > c0["handed_to_bicgstab"], (c0, c1)                # ... and a retry happened inside the replayed span
    env.set_state(s0)
    for _ in range(3):
        r2 = env.step(a)
    assert torch.equal(env._domain.velocity, u1) and torch.equal(env._domain.pressure, p1)
    assert torch.equal(r1[1], r2[1])
    env.close()


def test_env_step_is_the_per_step_smoothing_and_the_ordered_mean_of_the_wall_coefficients():
    """The env step (``mesh_body.MeshBodyEnvBase._step_impl``: the controls of all sim steps from the host recurrence, the wall forces
    in one buffer) against the sequence driven by hand on a second env: ``c + alpha (target - c)`` on the device, ``_apply_action``,
    ``_before_sim_step``, ``single_step``, ``_after_sim_step``, ``_get_drag_and_lift`` per sim step, their mean as adds in step order."""
    kw = dict(num_envs=2, resolution_div=2, initial_domain_steps=6, randomize_initial_state=False)
    action = torch.tensor([[0.8, -0.5, 0.3], [-0.2, 0.9, -0.6]], device="cuda")
    env = fluidgym_amd.make("Airfoil2D-easy-v0", **kw)
    env.reset(seed=0)
    assert float(env._last_control.abs().max()) == 0.0
    _, reward, _, _, info = env.step(action)
    hand = fluidgym_amd.make("Airfoil2D-easy-v0", **kw)
    hand.reset(seed=0)
    n, alpha = hand._n_sim_steps, hand._action_smoothing_alpha
    assert n == 5
    c, cds, cls = torch.zeros_like(action), [], []
    for k in range(n):
        c = c + alpha * (action - c)
        hand._apply_action(c)
        hand._before_sim_step(k)
        hand._sim.single_step()
        hand._after_sim_step()
        cd, cl = hand._get_drag_and_lift()
        cds.append(cd), cls.append(cl)
    assert torch.equal(env._last_control, c) and float(c.abs().min()) > 0
    cd, cl = cds[0].clone(), cls[0].clone()
    for k in range(1, n):
        cd += cds[k]
        cl += cls[k]
    cd /= n
    cl /= n
    assert torch.equal(info["drag"], cd) and torch.equal(info["lift"], cl)
    assert torch.equal(reward, cl / cd - env._cl_cd_ref)
    assert torch.equal(env._domain.velocity, hand._domain.velocity) and torch.equal(env._domain.pressure, hand._domain.pressure)
    env.close(), hand.close()
