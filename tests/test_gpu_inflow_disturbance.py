"""``fg_mb_inflow_disturbance`` on the GPU: on bare multi-block domains, in both libraries, the inflow rows and
the signals bit for bit against the NumPy restatement (``tests/inflow_disturbance_ref.py``), every other slot untouched, the outflow
scaled by one factor per env, the boundary fluxes balanced to the step's own guard; independence of the batch; and the cylinder and
airfoil envs with a disturbance started, stopped, reset per env, saved and restored."""
import functools

import numpy as np
import pytest
import torch

import fluidgym_amd
from fluidgym_amd.simulation.inflow_disturbance import InflowDisturbance
from tests import helpers_mb as H
from tests import inflow_disturbance_ref as R
from tests.test_gpu_cylinder import KW, KW3

pytestmark = pytest.mark.gpu

FLUX_BALANCE_TOL = 1e-5          # the guard at the top of fg_mb_single_step (MultiBlockSimulation's default)
B = 3
SIM_STEPS, K_SIM, DT = 5, 2, 0.0125
STEPS, EPISODES = [0, 3, 2_000_000], [0, 1, 7]      # n = 2, 17, 10^7 + 2
BAND, RMS_S, RMS_T, KAPPA, SEED = (0.05, 1.5), 0.1, 0.05, 0.7, 2 ** 40 + 11

# mesh -> (spec builder, inflow face, outflow face(s))
MESHES = {
    "split_rotated_channel": (H.split_rotated_channel, (0, 0), (1, 2)),
    "odd_channel_3d": (lambda: H.odd_channel_3d(nz=3), (0, 0), (1, 1)),
    "cylinder_2d": (lambda: H.cylinder_2d(res=8), (0, 0), (4, 1)),
    "airfoil": (lambda: H.airfoil_spec(div=4, balanced=True), (0, 0), [(4, 1), (5, 1)]),
}
INFLOW_SLOTS = {"split_rotated_channel": 8, "odd_channel_3d": 21}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


@functools.lru_cache(maxsize=None)
def _spec(mesh):
    return MESHES[mesh][0]()


@functools.lru_cache(maxsize=None)
def _domain(mesh, dtype, batch=B):
    return _spec(mesh).native(batch=batch, dtype=dtype)


def _counters(dom, steps, episodes):
    c = np.stack([np.asarray(steps, np.uint32), np.asarray(episodes, np.uint32)], axis=1)
    return torch.from_numpy(c.view(np.int32)).to(dom.boundary_velocity.device)


def _total_flux(dom, ub):
    """The signed boundary fluxes of every env summed over all slots, in fp64 from the handle's tables."""
    _, face, T = dom.boundary_tables()
    d = dom.dims
    T = T.astype(np.float64)
    axis = face >> 1
    w = np.stack([T[np.arange(len(face)), axis * d + c] for c in range(d)])              # [d, NB]
    w = w * (T[:, d * d] * np.where(face & 1, 1.0, -1.0))[None]
    return (ub.astype(np.float64) * w[None]).sum(axis=(1, 2))


def _table_spec(K, rng):
    u = lambda lo, hi: rng.uniform(lo, hi, (B, K))
    return InflowDisturbance(a=u(-0.1, 0.1), f=u(0.0, 2.0), phi=u(0.0, 1.0), g=u(-0.05, 0.05), h=u(0.0, 2.0), psi=u(0.0, 1.0), kappa=KAPPA)


def _modes_of(spec, batch, episodes):
    if spec.form == "random":
        return R.batch_modes(batch, spec.env_offset, episodes, spec.seed, spec.n_streamwise, spec.n_transverse, spec.band,
                             spec.streamwise_rms, spec.transverse_rms)
    t = spec.modes_table(batch)
    ks, kt = spec.n_streamwise, spec.n_transverse
    return [(t[b, 0, :ks].astype(np.float32), t[b, 1, :ks], t[b, 2, :ks], t[b, 3, :kt].astype(np.float32), t[b, 4, :kt], t[b, 5, :kt])
            for b in range(batch)]


def _check_launch(dom, inflow, outflow, spec, steps, episodes, start):
    """One launch from the boundary values ``start`` (which also serve as the base), every check of the module's docstring."""
    npdt = np.float32 if dom.boundary_velocity.dtype == torch.float32 else np.float64
    batch = dom.batch
    dom.boundary_velocity.copy_(start)
    base = start.clone()
    before = start.cpu().numpy()
    signal = dom.ApplyInflowDisturbance(inflow, outflow, base, spec, SIM_STEPS, K_SIM, _counters(dom, steps, episodes), DT, outflow_tol=5e-6)
    torch.cuda.synchronize()
    after, signal = dom.boundary_velocity.cpu().numpy(), signal.cpu().numpy()
    assert torch.equal(base, start)
    s0, cnt = dom._outflow_slots(inflow)
    ranges = [r for r in dom._outflow_ranges(outflow) if r[1] > 0]
    y = dom.face_centres(inflow)[1]
    y_mid = 0.5 * (float(y.min()) + float(y.max()))
    modes = _modes_of(spec, batch, episodes)
    touched = np.zeros(after.shape[2], bool)
    touched[s0:s0 + cnt] = True
    for b in range(batch):
        n = steps[b] * SIM_STEPS + K_SIM
        rows, sig = R.disturbance(modes[b], spec.kappa, n, DT, before[b][:, s0:s0 + cnt], y, y_mid, npdt)
        assert np.array_equal(_bits(after[b][:, s0:s0 + cnt]), _bits(rows)), f"inflow rows of env {b}"
        assert np.array_equal(_bits(signal[b]), _bits(sig)), f"signal of env {b}: {signal[b]} vs {sig}"
        for c in range(2, dom.dims):
            assert np.array_equal(_bits(after[b][c, s0:s0 + cnt]), _bits(before[b][c, s0:s0 + cnt]))
        # the outflow: one factor per env, taken where the old value is largest
        old = np.concatenate([before[b][:, r0:r0 + rn] for r0, rn in ranges], axis=1).astype(np.float64)
        new = np.concatenate([after[b][:, r0:r0 + rn] for r0, rn in ranges], axis=1)
        j = np.unravel_index(np.argmax(np.abs(old)), old.shape)
        factor = float(new[j]) / old[j]
        want = (factor * old).astype(npdt)
        assert np.all(np.abs(new - want) <= 4 * np.spacing(np.abs(want))), f"outflow of env {b} is not one factor times its previous values"
    for r0, rn in ranges:
        touched[r0:r0 + rn] = True
    assert np.array_equal(_bits(after[:, :, ~touched]), _bits(before[:, :, ~touched]))
    flux = _total_flux(dom, after)
    print(f"total boundary flux per env (fp64): {flux}")
    assert np.all(np.abs(flux) <= FLUX_BALANCE_TOL)
    return after, signal


@pytest.mark.parametrize("K", [0, 1, 8])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("mesh", list(MESHES))
def test_native_launch(mesh, dtype, K):
    dom = _domain(mesh, dtype)
    _, inflow, outflow = MESHES[mesh]
    snap = dom.Clone()
    start = snap["boundary_velocity"]
    if mesh in INFLOW_SLOTS:
        assert dom._outflow_slots(inflow)[1] == INFLOW_SLOTS[mesh]
    if mesh == "airfoil":
        assert sum(1 for r in dom._outflow_ranges(outflow) if r[1] > 0) == 2
    try:
        random = InflowDisturbance.random(SEED, K, K, BAND, RMS_S, RMS_T, kappa=KAPPA)
        after, signal = _check_launch(dom, inflow, outflow, random, STEPS, EPISODES, start)
        if K == 0:
            assert not signal.any()
        else:
            assert signal[:, 0].all() and len({float(s) for s in signal[:, 0]}) == B            # every env its own gust
        _check_launch(dom, inflow, outflow, _table_spec(K, np.random.default_rng(K)), STEPS, EPISODES, start)
        # the step's guard accepts what the launch left (a flux imbalance would raise with FG_ERR_FLUX_BALANCE's message)
        dom.single_step(0.01, adaptive=False, substeps=1, outflow=outflow, outflow_tol=5e-6, flux_balance_tol=FLUX_BALANCE_TOL,
                        max_iterations=300)
    finally:
        dom.Restore(snap)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_rows_do_not_depend_on_the_batch(dtype):
    """Rows 1..2 of a batch of 3 at offset 0 are a batch of 2 at offset 1, bit for bit: boundary values and signals."""
    _, inflow, outflow = MESHES["split_rotated_channel"]
    big, small = _domain("split_rotated_channel", dtype), _domain("split_rotated_channel", dtype, 2)
    out = []
    for dom, offset, sl in ((big, 0, slice(0, 3)), (small, 1, slice(1, 3))):
        snap = dom.Clone()
        try:
            spec = InflowDisturbance.random(SEED, 4, 3, BAND, RMS_S, RMS_T, kappa=KAPPA, env_offset=offset)
            base = snap["boundary_velocity"].clone()
            sig = dom.ApplyInflowDisturbance(inflow, outflow, base, spec, SIM_STEPS, K_SIM, _counters(dom, STEPS[sl], EPISODES[sl]), DT)
            out.append((dom.boundary_velocity.cpu().numpy(), sig.cpu().numpy()))
        finally:
            dom.Restore(snap)
    (ub3, sig3), (ub2, sig2) = out
    assert np.array_equal(_bits(ub3[1:]), _bits(ub2)) and np.array_equal(_bits(sig3[1:]), _bits(sig2))
    assert not np.array_equal(ub3[0], ub3[1])


# ---- the envs
RANDOM = dict(seed=31, n_streamwise=4, n_transverse=2, band=(0.2, 2.0), streamwise_rms=0.1, transverse_rms=0.03, kappa=0.25)


def _cylinder(num_envs=3):
    return fluidgym_amd.make("CylinderJet2D-easy-v0", num_envs=num_envs, **KW)


def _actions(env, scale=1.0):
    return scale * torch.linspace(-0.8, 0.6, env._zero_action.numel(), device=env.cuda_device).reshape(env._zero_action.shape)


def _fields(env):
    d = env._domain
    return [d.velocity.clone(), d.pressure.clone(), d.boundary_velocity.clone()]


def _inflow_rows(env):
    s0, cnt = env._domain._outflow_slots(env._mesh.inflow)
    return env._domain.boundary_velocity[:, :, s0:s0 + cnt].cpu().numpy()


def _expected(env, b, n, episode, kw=RANDOM):
    """Inflow rows and signal of env ``b`` at sim step ``n`` of episode ``episode`` by the restatement."""
    dom = env._domain
    s0, cnt = dom._outflow_slots(env._mesh.inflow)
    y = dom.face_centres(env._mesh.inflow)[1]
    modes = R.draw_modes(kw["seed"], b, episode, kw["n_streamwise"], kw["n_transverse"], kw["band"], kw["streamwise_rms"], kw["transverse_rms"])
    base = env._initial_boundary[b, :, s0:s0 + cnt].cpu().numpy()
    return R.disturbance(modes, kw["kappa"], n, env._sim.time_step, base, y, 0.5 * (float(y.min()) + float(y.max())), base.dtype.type)


def _same_step(r1, r2):
    return all(torch.equal(r1[0][k], r2[0][k]) for k in r1[0]) and torch.equal(r1[1], r2[1])


def test_env_start_stop_and_untouched_twin():
    env, twin = _cylinder(), _cylinder()
    env.reset(seed=0)
    with pytest.raises(RuntimeError, match="no inflow disturbance is active"):
        env.stop_inflow_disturbance()
    assert env.inflow_disturbance is None
    spec = env.start_inflow_disturbance(**RANDOM)
    assert env.inflow_disturbance is spec and spec.form == "random"
    _, _, _, _, info = env.step(_actions(env))
    assert "inflow" in info and info["inflow"].shape == (3, 2)
    s0, cnt = env._domain._outflow_slots(env._mesh.inflow)
    assert not np.array_equal(_inflow_rows(env), env._initial_boundary[:, :, s0:s0 + cnt].cpu().numpy())
    env.stop_inflow_disturbance()
    assert env.inflow_disturbance is None
    assert np.array_equal(_bits(_inflow_rows(env)), _bits(env._initial_boundary[:, :, s0:s0 + cnt].cpu().numpy()))
    assert np.all(np.abs(_total_flux(env._domain, env._domain.boundary_velocity.cpu().numpy())) <= FLUX_BALANCE_TOL)
    # started and stopped before reset: steps like an env that never started one
    env.reset(seed=0)
    twin.reset(seed=0)
    for _ in range(2):
        r1, r2 = env.step(_actions(env)), twin.step(_actions(twin))
        assert _same_step(r1, r2) and "inflow" not in r1[4]
    assert all(torch.equal(a, b) for a, b in zip(_fields(env), _fields(twin)))
    env.close(); twin.close()


def test_env_three_steps_info_and_per_env_reset():
    env = _cylinder()
    env.reset(seed=1)
    env.start_inflow_disturbance(**RANDOM)
    n_sim = env._n_sim_steps
    for _ in range(3):                               # the guard at the top of every sim step raises on an imbalance
        _, reward, _, _, info = env.step(_actions(env))
    assert torch.isfinite(reward).all()
    sig = info["inflow"].cpu().numpy()
    for b in range(3):
        rows, want = _expected(env, b, 2 * n_sim + n_sim - 1, 0)
        assert np.array_equal(_bits(sig[b]), _bits(want))
        assert np.array_equal(_bits(_inflow_rows(env)[b]), _bits(rows))
    assert torch.equal(env.inflow_signal(), info["inflow"])
    # a per-env reset: the others keep every bit, the chosen env starts episode 1 at t = 0
    before = _fields(env)
    env.reset_mesh_envs([1])
    after = _fields(env)
    for f0, f1 in zip(before, after):
        assert torch.equal(f0[0], f1[0]) and torch.equal(f0[2], f1[2])
    assert env.episode_steps.tolist() == [3, 0, 3] and env.mesh_reset_count.tolist() == [0, 1, 0]
    env._before_sim_step(0)
    rows = _inflow_rows(env)
    assert np.array_equal(_bits(rows[1]), _bits(_expected(env, 1, 0, 1)[0]))
    assert np.array_equal(_bits(rows[0]), _bits(_expected(env, 0, 3 * n_sim, 0)[0]))
    assert np.array_equal(_bits(rows[2]), _bits(_expected(env, 2, 3 * n_sim, 0)[0]))
    env.close()


def test_env_state_replays():
    env = _cylinder()
    env.reset(seed=2)
    env.start_inflow_disturbance(InflowDisturbance(a=[[0.1, 0.05], [0.2, 0.0], [0.0, 0.1]], f=[0.7, 1.9], phi=[0.1, 0.6], g=[0.04], h=[1.1], psi=[0.3], kappa=0.5))
    env.step(_actions(env))
    state = env.get_state()
    assert state["extra"]["inflow_disturbance"]["form"] == "tables"
    first = [env.step(_actions(env, s)) for s in (1.0, -0.5)]
    fields = _fields(env)
    env.stop_inflow_disturbance()
    env.set_state(state)
    assert env.inflow_disturbance is not None and env.inflow_disturbance.n_streamwise == 2
    second = [env.step(_actions(env, s)) for s in (1.0, -0.5)]
    for r1, r2 in zip(first, second):
        assert _same_step(r1, r2) and torch.equal(r1[4]["inflow"], r2[4]["inflow"])
    assert all(torch.equal(a, b) for a, b in zip(fields, _fields(env)))
    env.close()


def _smoke(env, nz=1):
    env.reset(seed=3)
    kw = dict(RANDOM, streamwise_rms=0.1)
    env.start_inflow_disturbance(**kw)
    _, reward, _, _, info = env.step(_actions(env, 0.5))
    assert torch.isfinite(reward).all()
    sig, rows, n_sim = info["inflow"].cpu().numpy(), _inflow_rows(env), env._n_sim_steps
    for b in range(env.num_envs):
        want_rows, want = _expected(env, b, n_sim - 1, 0, kw)
        assert np.array_equal(_bits(sig[b]), _bits(want)) and np.array_equal(_bits(rows[b]), _bits(want_rows))
    assert sig[:, 0].all()
    layers = rows.reshape(rows.shape[0], rows.shape[1], nz, -1)
    assert np.array_equal(_bits(layers), _bits(np.broadcast_to(layers[:, :, :1], layers.shape)))       # constant along z
    assert np.all(np.abs(_total_flux(env._domain, env._domain.boundary_velocity.cpu().numpy())) <= FLUX_BALANCE_TOL)
    env.stop_inflow_disturbance()
    env.close()


def test_env_cylinder_3d():
    _smoke(fluidgym_amd.make("CylinderJet3D-easy-v0", num_envs=2, **KW3), nz=KW3["resolution"])


def test_env_airfoil():
    from tests.test_gpu_mb_tracers import _airfoil

    _smoke(_airfoil())


def test_refusals_on_single_block_and_parallel_envs():
    from fluidgym_amd.envs.parallel_env import ParallelFluidEnv

    rbc = fluidgym_amd.make("RBC2D-easy-v0", num_envs=2, n_heaters=4, resolution=8, step_length=0.1, load_initial_domain=False,
                            load_domain_statistics=False, randomize_initial_state=False)
    rbc.reset(seed=7)
    assert rbc.inflow_disturbance is None
    for call in (lambda: rbc.start_inflow_disturbance(**RANDOM), rbc.stop_inflow_disturbance, rbc.inflow_signal):
        with pytest.raises(NotImplementedError, match="cylinder, airfoil"):
            call()
    rbc.close()
    penv = ParallelFluidEnv("CylinderJet2D-easy-v0", cuda_ids=[0], num_envs=2, **KW)
    for call in (lambda: penv.start_inflow_disturbance(**RANDOM), penv.stop_inflow_disturbance, penv.inflow_signal):
        with pytest.raises(NotImplementedError, match="ParallelFluidEnv"):
            call()
    penv.close()
