"""The after-sim-step hook list on the envs (``envs/step_hooks.py``): every consumer of an env active at once, started in reverse of the
canonical order, counts what its ``every`` says, leaves observations and rewards alone and records the bits it records when it is the
only one; the clouds travel through ``get_state`` / ``set_state`` under their keys."""
import functools

import pytest
import torch

import fluidgym_amd
from fluidgym_amd.simulation.mb_tracers import MeshTracerCloud
from fluidgym_amd.simulation.tracers import TracerCloud

pytestmark = pytest.mark.gpu

# the TCF of tests/test_gpu_flow_statistics.py and the cylinder of tests/test_gpu_field_statistics.py
TCF = dict(num_envs=2, randomize_initial_state=False, resolution_x_z=16, resolution_y=16, step_length=0.6, use_marl=False)
KW = dict(resolution=8, initial_domain_steps=6, randomize_initial_state=False, step_length=0.05, dt=0.01, episode_length=3)
STEPS, N_TRACERS = 2, 8

# consumer -> (every, start, stop); in the canonical order, every = 1, 2, 1, 2, 1, 2
SINGLE = {
    "flow_stats": (1, lambda e, k: e.start_flow_statistics(order=2, every=k), lambda e: e.stop_flow_statistics()),
    "flow_spectra": (2, lambda e, k: e.start_flow_spectra((5, 1), every=k), lambda e: e.stop_flow_spectra()),
    "flow_budgets": (1, lambda e, k: e.start_flow_budgets(every=k), lambda e: e.stop_flow_budgets()),
    "flow_timecorr": (2, lambda e, k: e.start_flow_time_correlation(lags=4, every=k, stride=2), lambda e: e.stop_flow_time_correlation()),
    "flow_hist": (1, lambda e, k: e.start_flow_histograms(bins=64, every=k), lambda e: e.stop_flow_histograms()),
    "tracers": (2, lambda e, k: e.start_tracers(N_TRACERS, seed=5, every=k), lambda e: e.stop_tracers()),
}
MULTI = {
    "field_stats": (2, lambda e, k: e.start_field_statistics(every=k), lambda e: e.stop_field_statistics()),
    "mesh_tracers": (1, lambda e, k: e.start_mesh_tracers(N_TRACERS, seed=0, every=k), lambda e: e.stop_mesh_tracers()),
}
FAMILY = {"single": ("TCFSmall3D-both-easy-v0", TCF, SINGLE), "multi": ("CylinderJet2D-easy-v0", dict(KW, num_envs=2), MULTI)}


def _tensors(x):
    if isinstance(x, dict):
        return [t for k in sorted(x) for t in _tensors(x[k])]
    return [t for v in x for t in _tensors(v)] if isinstance(x, (tuple, list)) else [x]


def _bits(record):
    """What a record holds, as bytes: the state arrays of a recorder, the state tensors of a cloud."""
    if isinstance(record, (TracerCloud, MeshTracerCloud)):
        return [getattr(record, k).cpu().numpy().tobytes() for k in record._STATE]
    state = record._state()
    return [a.tobytes() for a in (state if isinstance(state, tuple) else (state,))]


@functools.lru_cache(maxsize=None)
def _run(family, active):
    """``STEPS`` env steps under seeded actions with the consumers ``active`` started in reverse canonical order: the records, how
    often each cloud was advanced, observations and rewards, the sim steps per env step and the grid."""
    env_id, kw, consumers = FAMILY[family]
    env = fluidgym_amd.make(env_id, **kw)
    env.reset(seed=4)
    advances = {}
    for name in reversed(active):
        every, start, _ = consumers[name]
        cloud = start(env, every)
        if cloud is not None:                        # count the launches of a cloud: it has no sample counter of its own
            advect, advances[name] = cloud.advect, []
            cloud.advect = lambda dt, advect=advect, calls=advances[name]: (calls.append(dt), advect(dt))
    assert list(env._step_hooks) == list(active)
    gen = torch.Generator().manual_seed(0)
    outs = []
    for _ in range(STEPS):
        a = (torch.rand(env._zero_action.shape, generator=gen) * 2 - 1).to(env.cuda_device, env._dtype)
        outs.append([t.clone() for t in _tensors(env.step(a)[:2])])
    records = {name: consumers[name][2](env) for name in active}
    assert not env._step_hooks
    sim_steps = env._n_sim_steps
    env.close()
    return records, {k: len(v) for k, v in advances.items()}, outs, sim_steps


def _samples(name, record, advances):
    """How many samples the record took, from its own counter."""
    if name in ("tracers", "mesh_tracers"):
        return advances[name]
    if name in ("flow_stats", "flow_budgets"):       # n: cells seen per row and env = samples x nz x nx
        n = record.n.tolist()
        assert n == [n[0]] * 2 and n[0] % (16 * 16) == 0
        return int(n[0]) // (16 * 16)
    return record.n_samples if name == "flow_hist" else record.samples


@pytest.mark.parametrize("family", ["single", "multi"])
def test_all_consumers_at_once_count_by_their_every_and_leave_the_step_alone(family):
    consumers = FAMILY[family][2]
    records, advances, outs, sim_steps = _run(family, tuple(consumers))
    for name, record in records.items():
        every = consumers[name][0]
        print(name, "every", every, "samples", _samples(name, record, advances), "of", STEPS * sim_steps, "sim steps")
        assert _samples(name, record, advances) == (STEPS * sim_steps) // every
    _, _, plain, _ = _run(family, ())
    assert len(outs) == len(plain) == STEPS
    for with_all, without in zip(outs, plain):
        assert len(with_all) == len(without) and all(torch.equal(a, b) for a, b in zip(with_all, without))


@pytest.mark.parametrize("family, name", [(f, n) for f in FAMILY for n in FAMILY[f][2]])
def test_a_consumer_among_all_records_the_bits_it_records_alone(family, name):
    together, _, _, _ = _run(family, tuple(FAMILY[family][2]))
    alone, advances, _, sim_steps = _run(family, (name,))
    assert _samples(name, alone[name], advances) == (STEPS * sim_steps) // FAMILY[family][2][name][0]
    assert _bits(together[name]) == _bits(alone[name])


@pytest.mark.parametrize("family", ["single", "multi"])
def test_a_cloud_travels_in_the_state_under_its_key_and_replays(family):
    env_id, kw, consumers = FAMILY[family]
    key, cls = ("tracers", TracerCloud) if family == "single" else ("mesh_tracers", MeshTracerCloud)
    scalars = {"substeps", "respawn_faces"} if family == "single" else {"substeps"}
    env = fluidgym_amd.make(env_id, **kw)
    env.reset(seed=4)
    assert key not in env.get_state()
    cloud = consumers[key][1](env, 2)
    zero = torch.zeros(env._zero_action.shape, device=env.cuda_device)
    env.step(zero)
    state = env.get_state()
    assert set(state) == {"domain", "n_steps", "extra", key} and set(state[key]) == {"cloud", "every", "tick"}
    assert set(state[key]["cloud"]) == set(cls._STATE) | scalars
    assert (state[key]["every"], state[key]["tick"]) == (2, env._n_sim_steps)
    env.step(zero)
    before = {k: getattr(cloud, k).clone() for k in cls._STATE}
    assert not torch.equal(before["positions"], state[key]["cloud"]["positions"])
    env.set_state(state)
    assert torch.equal(cloud.positions, state[key]["cloud"]["positions"]) and env._step_hooks[key].tick == env._n_sim_steps
    env.step(zero)
    assert all(torch.equal(getattr(cloud, k), before[k]) for k in cls._STATE)
    consumers[key][2](env)
    with pytest.raises(RuntimeError, match="none is active"):
        env.set_state(state)
    env.close()
