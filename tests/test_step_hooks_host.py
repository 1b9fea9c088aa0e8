"""The after-sim-step hook list of the envs (``envs/step_hooks.py``) on the host: a stub env that derives from the mixin and goes through
it the way ``FluidEnv`` does, with plain Python targets.  No library, no GPU."""
import itertools

import pytest

from fluidgym_amd.envs.step_hooks import HOOK_ORDER, STATE_KEYS, StepHooksMixin


class Target:
    """Counts its runs; a cloud's reseed / state_dict / load_state_dict in plain Python."""

    def __init__(self, log=None, name=""):
        self.runs, self.reseeds, self.value, self.log, self.name = 0, [], 0, log, name

    def run(self):
        self.runs += 1
        self.value += 1
        if self.log is not None:
            self.log.append(self.name)

    def reseed(self, envs=None):
        self.reseeds.append(envs)
        self.value = 0

    def state_dict(self):
        return {"value": self.value}

    def load_state_dict(self, state):
        self.value = state["value"]


class StubEnv(StepHooksMixin):
    """The calls ``FluidEnv`` makes, without a simulation."""

    def start(self, name, target, every=1, cloud=False):
        extra = dict(reseed=target.reseed, state_key=name) if cloud else {}
        return self._start_hook(name, target, every, target.run, **extra)

    def step(self, n=1):
        for _ in range(n):
            self._after_sim_step()

    def reset(self):
        self._reseed_hooks()

    def reset_envs(self, envs):
        self._reseed_hooks(envs)

    def get_state(self):
        return {"n_steps": 0, **self._hooks_state()}

    def set_state(self, state):
        self._load_hooks_state(state)

    def close(self):
        self._step_hooks = {}


def test_the_order_is_the_ladders_and_the_state_keys_are_hooks():
    assert HOOK_ORDER == ("flow_stats", "flow_spectra", "flow_budgets", "flow_timecorr", "flow_hist", "field_stats", "tracers",
                          "mesh_tracers")
    assert set(STATE_KEYS) == {"tracers", "mesh_tracers"}
    assert not StubEnv()._step_hooks and StubEnv()._hook("tracers") is None


@pytest.mark.parametrize("started", list(itertools.permutations(("flow_spectra", "flow_hist", "tracers"))))
def test_hooks_run_in_the_canonical_order_whatever_order_they_were_started_in(started):
    env, log = StubEnv(), []
    for name in started:
        env.start(name, Target(log, name))
    env.step(2)
    assert log == ["flow_spectra", "flow_hist", "tracers"] * 2 and list(env._step_hooks) == ["flow_spectra", "flow_hist", "tracers"]
    assert StubEnv()._step_hooks == {}                                      # another env sees nothing of it


@pytest.mark.parametrize("every", [1, 2, 3])
def test_every_and_tick_over_seven_steps(every):
    env, t = StubEnv(), Target()
    assert env.start("flow_stats", t, every) is t
    runs = []
    for _ in range(7):
        env.step()
        runs.append(t.runs)
    assert runs == [k // every for k in range(1, 8)] and env._step_hooks["flow_stats"].tick == 7
    assert env._step_hooks["flow_stats"].every == every


@pytest.mark.parametrize("every", [0, -1])
def test_every_below_one_is_refused_once_for_all(every):
    env = StubEnv()
    with pytest.raises(ValueError, match=f"every must be at least 1, got {every}"):
        env.start("flow_budgets", Target(), every)
    with pytest.raises(KeyError, match="HOOK_ORDER"):                      # a new consumer takes its place in the order first
        env.start("ninth", Target())
    assert not env._step_hooks


def test_stop_hands_out_the_target_and_raises_the_second_time():
    env, t, other = StubEnv(), Target(), Target()
    env.start("flow_budgets", t)
    env.start("tracers", other)
    assert env._hook("flow_budgets") is t
    assert env._stop_hook("flow_budgets", "stop_flow_budgets: no budgets are being recorded") is t
    assert env._hook("flow_budgets") is None and env._hook("tracers") is other
    with pytest.raises(RuntimeError, match="no budgets are being recorded"):
        env._stop_hook("flow_budgets", "stop_flow_budgets: no budgets are being recorded")
    env.step()
    assert t.runs == 0 and other.runs == 1


def test_starting_an_active_name_replaces_the_hook_and_zeroes_its_tick():
    env, old, new = StubEnv(), Target(), Target()
    env.start("flow_hist", old, every=2)
    env.step(3)
    assert env._step_hooks["flow_hist"].tick == 3 and old.runs == 1
    env.start("flow_hist", new, every=2)
    assert env._hook("flow_hist") is new and env._step_hooks["flow_hist"].tick == 0 and len(env._step_hooks) == 1
    env.step(2)
    assert old.runs == 1 and new.runs == 1


def test_reset_reseeds_all_and_zeroes_the_tick_reset_envs_the_chosen_and_keeps_it():
    env, cloud, recorder = StubEnv(), Target(), Target()
    env.start("tracers", cloud, every=3, cloud=True)
    env.start("flow_stats", recorder, every=3)
    env.step(2)
    env.reset_envs([1])
    assert cloud.reseeds == [[1]] and env._step_hooks["tracers"].tick == 2
    env.reset()
    assert cloud.reseeds == [[1], None] and env._step_hooks["tracers"].tick == 0
    assert recorder.reseeds == [] and env._step_hooks["flow_stats"].tick == 2      # a recorder has no seeds: it keeps counting
    env.step(2)
    assert cloud.runs == 0 and recorder.runs == 1


def test_state_round_trip_through_the_state_key():
    env, cloud, mesh_cloud, recorder = StubEnv(), Target(), Target(), Target()
    env.start("tracers", cloud, every=2, cloud=True)
    env.start("mesh_tracers", mesh_cloud, every=3, cloud=True)
    env.start("flow_stats", recorder)
    env.step(3)
    state = env.get_state()
    assert set(state) == {"n_steps", "tracers", "mesh_tracers"}                    # recorders do not travel
    assert state["tracers"] == {"cloud": {"value": 1}, "every": 2, "tick": 3}
    assert state["mesh_tracers"] == {"cloud": {"value": 1}, "every": 3, "tick": 3}
    env.step(1)
    assert cloud.value == 2
    env.set_state(state)
    assert cloud.value == 1 and env._step_hooks["tracers"].tick == 3 and env._step_hooks["tracers"].every == 2
    env.step(1)
    assert cloud.value == 2                                                        # the step after set_state is the step taken before
    # another env with a cloud started at another period takes the state's period
    twin, twin_cloud = StubEnv(), Target()
    twin.start("tracers", twin_cloud, every=5, cloud=True)
    twin.set_state({"tracers": state["tracers"]})
    assert twin_cloud.value == 1 and (twin._step_hooks["tracers"].every, twin._step_hooks["tracers"].tick) == (2, 3)


@pytest.mark.parametrize("key, what, entry", [("tracers", "tracer cloud", "start_tracers"),
                                              ("mesh_tracers", "mesh tracer cloud", "start_mesh_tracers")])
def test_a_state_with_a_cloud_needs_an_active_one(key, what, entry):
    env, cloud = StubEnv(), Target()
    env.start(key, cloud, cloud=True)
    state = env.get_state()
    env._stop_hook(key, "stop: no tracers are active")
    assert key not in env.get_state()
    with pytest.raises(RuntimeError, match=rf"holds a {what} but none is active; call {entry}\(\)"):
        env.set_state(state)
    env.set_state({"n_steps": 0})                                                  # a state without a cloud asks for none


def test_close_empties_the_list():
    env, t = StubEnv(), Target()
    env.start("field_stats", t)
    env.start("mesh_tracers", Target(), cloud=True)
    env.close()
    assert not env._step_hooks and env._hook("field_stats") is None and env.get_state() == {"n_steps": 0}
    env.step()
    assert t.runs == 0
