"""SHA-256 digests of what the per-sim-step consumers of the envs record, to compare two commits on one machine: every consumer of a
single-block env at once (TCF 16^3), field statistics and mesh tracers of the 2-D cylinder, and a tracer cloud in the channel env.
Only public entry points are used, so the same file runs at either commit.  One JSON line: name -> digest.
python profiles/step_hooks_ab.py"""
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fluidgym_amd  # noqa: E402

TCF = dict(num_envs=2, randomize_initial_state=False, resolution_x_z=16, resolution_y=16, step_length=0.6, use_marl=False)
CYL = dict(num_envs=2, resolution=8, initial_domain_steps=6, randomize_initial_state=False, step_length=0.05, dt=0.01, episode_length=3)
CHANNEL = dict(num_envs=2, resolution_x=64, resolution_y=32, randomize_initial_state=False, load_initial_domain=False,
               load_domain_statistics=False)


def digest(*arrays) -> str:
    h = hashlib.sha256()
    for a in arrays:
        a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
        h.update(str((a.dtype, a.shape)).encode())
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def flat(x):
    """The tensors of an observation / reward (a dict, a tuple or a tensor), in a fixed order."""
    if isinstance(x, dict):
        return [t for k in sorted(x) for t in flat(x[k])]
    if isinstance(x, (tuple, list)):
        return [t for v in x for t in flat(v)]
    return [x]


def state_arrays(record):
    s = record._state()
    return list(s) if isinstance(s, tuple) else [s]


def cloud_arrays(cloud):
    return [getattr(cloud, k) for k in type(cloud)._STATE]


def run(env_id, kw, seed, start, steps=2):
    """``steps`` env steps under the zero action after ``start(env)``; the digests of observations and rewards, and the env."""
    env = fluidgym_amd.make(env_id, **kw)
    env.reset(seed=seed)
    start(env)
    zero = torch.zeros(env._zero_action.shape, device=env.cuda_device)
    outs = [env.step(zero)[:2] for _ in range(steps)]
    return env, digest(*flat(outs))


out = {}

# every single-block consumer at once, started in reverse order
def all_six(env):
    env.start_tracers(8, seed=5, every=2)
    env.start_flow_histograms(bins=64, every=1)
    env.start_flow_time_correlation(lags=4, every=2, stride=2)
    env.start_flow_budgets(every=1)
    env.start_flow_spectra((5, 1), every=2)
    env.start_flow_statistics(order=2, every=1)

env, out["tcf/obs_reward"] = run("TCFSmall3D-both-easy-v0", TCF, 4, all_six)
out["tcf/flow_stats"] = digest(*state_arrays(env.stop_flow_statistics()))
out["tcf/flow_spectra"] = digest(*state_arrays(env.stop_flow_spectra()))
out["tcf/flow_budgets"] = digest(*state_arrays(env.stop_flow_budgets()))
out["tcf/flow_timecorr"] = digest(*state_arrays(env.stop_flow_time_correlation()))
out["tcf/flow_hist"] = digest(*state_arrays(env.stop_flow_histograms()))
out["tcf/tracers"] = digest(*cloud_arrays(env.stop_tracers()))
env.close()

# field statistics and mesh tracers of the cylinder
def both(env):
    env.start_mesh_tracers(8, seed=0, every=1)
    env.start_field_statistics(every=2)

env, out["cylinder/obs_reward"] = run("CylinderJet2D-easy-v0", CYL, 4, both)
out["cylinder/field_stats"] = digest(*state_arrays(env.stop_field_statistics()))
out["cylinder/mesh_tracers"] = digest(*cloud_arrays(env.stop_mesh_tracers()))
env.close()

# a tracer cloud in the channel env: its sim steps run one by one while the cloud is active
env, out["channel/obs_reward"] = run("ChannelJet2D-v0", CHANNEL, 2, lambda e: e.start_tracers(8, seed=1, every=1))
out["channel/velocity"] = digest(env._domain.getBlock(0).velocity)
out["channel/tracers"] = digest(*cloud_arrays(env.stop_tracers()))
env.close()

print(json.dumps(out))
