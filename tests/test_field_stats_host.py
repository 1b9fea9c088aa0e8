"""Domain statistics without a GPU: the range-doubling histogram against ``np.histogram``, the ``Stats`` file format, what a
statistics file on disk does to the reward references of every env family, and the ABI of ``fg_field_summary``."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import fluidgym_amd
from fluidgym_amd import _lib as L
from fluidgym_amd.simulation.field_stats import HistogramRange, HostFieldSummary, bin_index
from fluidgym_amd.types import EnvMode, Stats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("mean", "min", "max", "p5", "p25", "p50", "p75", "p95")


def _stats(seed: float) -> dict:
    return {k: seed + 0.125 * i for i, k in enumerate(FIELDS)}


def _write(root, env, payload) -> str:
    d = root / "initial_domains" / env.initial_domain_id
    d.mkdir(parents=True, exist_ok=True)
    with open(d / "domain_statistics.json", "w") as f:
        json.dump(payload, f, indent=4)
    return str(d / "domain_statistics.json")


@pytest.fixture
def data_path(tmp_path, monkeypatch):
    monkeypatch.setenv("FLUIDGYM_DATA_PATH", str(tmp_path))
    monkeypatch.setitem(fluidgym_amd.config.settings, "local_data_path", None)
    return tmp_path


def test_range_doubling_accumulator_equals_numpy_histogram():
    """2e5 half-normal samples in 50 chunks, starting from a range that fits only the first 1000: the folded counts are the
    counts of one histogram of everything over the final range, and the quantiles are within one final bin width."""
    x = np.abs(np.random.default_rng(7).standard_normal(200_000))
    acc = HostFieldSummary(nbins=2048)
    acc.update(x[:1000].reshape(1, 1, -1), channel=0)
    first = (acc.range.lo, acc.range.width)
    assert x[:1000].max() < acc.range.hi <= x.max()          # the start range really is too small for the rest
    for chunk in np.array_split(x[1000:], 49):
        acc.update(chunk.reshape(1, 1, -1), channel=0)
    r = acc.range
    assert r.width > first[1] and np.log2(r.width / first[1]) == int(np.log2(r.width / first[1]))
    ref, edges = np.histogram(x, bins=r.nbins, range=(r.lo, r.hi))
    assert np.array_equal(edges, r.lo + r.width * np.arange(r.nbins + 1))       # every edge is an exact number
    assert np.array_equal(acc.histogram(), ref)
    assert np.array_equal(np.bincount(bin_index(x, r.lo, r.width, r.nbins), minlength=r.nbins), ref)
    st = acc.stats()
    assert st.min == x.min() and st.max == x.max() and st.mean == pytest.approx(x.mean(), rel=1e-13)
    err = np.abs(np.array(st[3:]) - np.quantile(x, [0.05, 0.25, 0.5, 0.75, 0.95])) / r.width
    print("quantile errors in bin widths:", err)
    assert err.max() <= 1.0


def test_range_grows_downward_without_losing_counts():
    y = np.random.default_rng(8).standard_normal(40_000)
    order = np.argsort(-y)                                    # descending: every chunk reaches further down
    acc = HostFieldSummary(nbins=256, per_env=True)
    for chunk in np.array_split(y[order], 8):
        acc.update(chunk.reshape(2, 1, -1), channel=0)
    r = acc.range
    assert np.array_equal(acc.histogram().sum(axis=0), np.histogram(y, bins=r.nbins, range=(r.lo, r.hi))[0])
    assert acc.count == y.size and [s.min for s in acc.stats()] == [chunk.min() for chunk in
                                                                     (y[order].reshape(8, 2, -1)[:, b].ravel() for b in range(2))]
    # folding: pairs merge into one half, the other half is zero, nothing is lost
    h = np.arange(1, 9)
    assert HistogramRange.fold(h, "up").tolist() == [3, 7, 11, 15, 0, 0, 0, 0]
    assert HistogramRange.fold(h, "down").tolist() == [0, 0, 0, 0, 3, 7, 11, 15]
    assert HistogramRange.fold(torch.as_tensor(h), "down").tolist() == [0, 0, 0, 0, 3, 7, 11, 15]


def test_constant_field_and_magnitude_and_merge():
    c = HostFieldSummary(nbins=64)
    c.update(np.full((2, 1, 50), -3.25), channel=0)
    assert c.range.width > 0 and np.count_nonzero(c.histogram()) == 1 and c.histogram().sum() == 100
    assert c.stats() == Stats(*([-3.25] * 8))
    rng = np.random.default_rng(9)
    u = rng.standard_normal((3, 2, 4000))
    a, b = HostFieldSummary(nbins=512), HostFieldSummary(nbins=512)
    a.update(u[:, :, :1000]), b.update(3.0 * u[:, :, 1000:])          # magnitudes: both grids start at 0, so they nest
    assert a.range.lo == 0.0 and b.range.lo == 0.0
    a.merge(b)
    mag = np.concatenate([np.hypot(*np.moveaxis(u[:, :, :1000], 1, 0)).ravel(), 3.0 * np.hypot(*np.moveaxis(u[:, :, 1000:], 1, 0)).ravel()])
    r = a.range
    assert np.array_equal(a.histogram(), np.histogram(mag, bins=r.nbins, range=(r.lo, r.hi))[0])
    assert a.stats().max == pytest.approx(mag.max(), rel=1e-15) and a.stats().mean == pytest.approx(mag.mean(), rel=1e-12)
    with pytest.raises(ValueError, match="nbins"):
        HostFieldSummary(nbins=4097)


def test_stats_json_round_trip(tmp_path):
    s = Stats(mean=0.1, min=-1.0 / 3.0, max=2.0 ** 0.5, p5=-0.3, p25=0.0, p50=1e-17, p75=0.7, p95=1.25)
    assert Stats._fields == FIELDS
    path = tmp_path / "s.json"
    with open(path, "w") as f:
        json.dump({"x": s._asdict()}, f, indent=4)
    assert Stats(**json.load(open(path))["x"]) == s


def test_statistics_file_loads_without_vorticity_and_names_a_missing_key(data_path):
    env = fluidgym_amd.make("RBC2D-easy-v0", cuda_device="cpu")
    assert env.nu_ref == 0.0 and env._velocity_stats is None
    full = {"velocity_magnitude": _stats(1.0), "pressure": _stats(2.0), "nusselt": _stats(3.0)}      # no vorticity_magnitude
    _write(data_path, env, full)
    assert env.nu_ref == 0.0                                  # this env looked already: a file is picked up by the next one
    env = fluidgym_amd.make("RBC2D-easy-v0", cuda_device="cpu")
    assert env._metrics_stats == {}                           # the constructor reads nothing
    env._ensure_domain_statistics()
    assert env._metrics_stats == {"nusselt": Stats(**_stats(3.0))}
    assert env._velocity_stats == Stats(**_stats(1.0)) and env._pressure_stats.p95 == 2.0 + 0.125 * 7
    for missing in ("pressure", "velocity_magnitude", "nusselt"):
        _write(data_path, env, {k: v for k, v in full.items() if k != missing})
        with pytest.raises(KeyError, match=missing):
            fluidgym_amd.make("RBC2D-easy-v0", cuda_device="cpu").nu_ref
    # load_domain_statistics=False never looks
    assert fluidgym_amd.make("RBC2D-easy-v0", cuda_device="cpu", load_domain_statistics=False).nu_ref == 0.0


def test_the_first_reset_loads_the_file(data_path, monkeypatch):
    """A real registry env on the CPU stand-in solver (tests/stub_solver.py), as the gloo tests run it: reset() is where the file
    is read, so a file without ``pressure`` fails there, and a complete one fills the three records."""
    import fluidgym_amd.simulation.domain as D
    from tests.stub_solver import StubSolver

    monkeypatch.setattr(D, "NativeSolver", StubSolver)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)        # FluidEnv.reset's guard; nothing here touches a GPU
    kw = dict(cuda_device="cpu", randomize_initial_state=False, resolution_x=32, resolution_y=16, step_length=0.05,
              load_domain_statistics=True, load_initial_domain=False)
    env = fluidgym_amd.make("ChannelJet2D-v0", **kw)
    full = {"velocity_magnitude": _stats(1.0), "pressure": _stats(2.0), "cross_flow_energy": _stats(3.0), "wall_shear": _stats(4.0)}
    _write(data_path, env, {k: v for k, v in full.items() if k != "pressure"})
    with pytest.raises(KeyError, match="pressure"):
        env.reset(seed=0)
    _write(data_path, env, full)
    env = fluidgym_amd.make("ChannelJet2D-v0", **kw)
    assert env._pressure_stats is None
    env.reset(seed=0)
    assert env._pressure_stats == Stats(**_stats(2.0)) and env._metrics_stats["wall_shear"].mean == 4.0
    assert env.get_uncontrolled_episode_metrics() is None


def test_reward_references_follow_the_reference_rules(data_path, monkeypatch):
    mk = lambda env_id, **kw: fluidgym_amd.make(env_id, cuda_device="cpu", **kw)
    base = {"velocity_magnitude": _stats(1.0), "pressure": _stats(2.0)}
    cases = [   # env id, metrics in the file, (attribute, value without a file, value with it)
        ("RBC2D-easy-v0", {"nusselt": _stats(3.0)}, ("nu_ref", 0.0, 3.0 + 0.125 * 5)),                    # p50 in 2-D
        ("RBC3D-easy-v0", {"nusselt": _stats(3.0)}, ("nu_ref", 0.0, 3.0)),                                # mean in 3-D
        ("TCFSmall3D-bottom-easy-v0", {"wall_stress": _stats(5.0), "wall_stress_bottom": _stats(6.0), "wall_stress_top": _stats(7.0)},
         ("tau_ref", 1.0, 6.0)),
        ("TCFSmall3D-both-easy-v0", {"wall_stress": _stats(5.0), "wall_stress_bottom": _stats(6.0), "wall_stress_top": _stats(7.0)},
         ("tau_ref", 1.0, 5.0)),
        ("CylinderJet2D-easy-v0", {"drag": _stats(3.5), "lift": _stats(0.25)}, ("_cd_ref", 0.0, 3.5)),
        ("CylinderRot2D-easy-v0", {"drag": _stats(3.5), "lift": _stats(0.25)}, ("_cd_ref", 0.0, 3.5)),
        ("CylinderJet3D-easy-v0", {"drag": _stats(3.5), "lift": _stats(0.25)}, ("_cd_ref", 0.0, 3.5)),
        ("Airfoil2D-easy-v0", {"drag": _stats(0.5), "lift": _stats(1.5)}, ("_cl_cd_ref", 0.0, 3.0)),
        ("Airfoil3D-easy-v0", {"drag": _stats(0.5), "lift": _stats(1.5)}, ("_cl_cd_ref", 0.0, 3.0)),
    ]
    ids = [i for i in fluidgym_amd.registry.ids]
    for env_id, metrics, (attr, without, with_file) in cases:
        assert env_id in ids, env_id
        root = data_path / env_id                                # (several ids share one initial_domain_id: a directory each)
        monkeypatch.setenv("FLUIDGYM_DATA_PATH", str(root))
        env = mk(env_id)
        assert getattr(env, attr) == without, (env_id, "no file")
        _write(root, env, {**base, **metrics})
        assert getattr(env, attr) == without                     # looked once, before the file existed
        env = mk(env_id)
        assert getattr(env, attr) == with_file, (env_id, "with file")
        assert getattr(mk(env_id, load_domain_statistics=False), attr) == without
    # 3-D airfoil: drag and abs_lift references as in the reference (abs_lift is no metric of the env, so it stays 0)
    a3 = mk("Airfoil3D-easy-v0")
    assert a3._cd_ref == 0.5 and a3._cl_ref == 0.0
    # an explicit non-zero reference still wins; an explicit zero does not
    monkeypatch.setenv("FLUIDGYM_DATA_PATH", str(data_path / "CylinderJet2D-easy-v0"))
    assert mk("CylinderJet2D-easy-v0", drag_reference=2.25)._cd_ref == 2.25
    assert mk("CylinderJet2D-easy-v0", drag_reference=0.0)._cd_ref == 3.5
    monkeypatch.setenv("FLUIDGYM_DATA_PATH", str(data_path / "Airfoil2D-easy-v0"))
    assert mk("Airfoil2D-easy-v0", lift_drag_reference=7.0)._cl_cd_ref == 7.0
    monkeypatch.setenv("FLUIDGYM_DATA_PATH", str(data_path / "RBC2D-easy-v0"))
    # a batch with per-env parameters has no id, hence no file: today's value
    assert mk("RBC2D-easy-v0", num_envs=2, rayleigh_number=[8e4, 4e5]).nu_ref == 0.0


def test_uncontrolled_episode_csv_is_returned_after_a_reset_that_loaded_the_domain(data_path):
    env = fluidgym_amd.make("RBC2D-easy-v0", cuda_device="cpu")
    d = env._get_domain_dir(0)
    d.mkdir(parents=True)
    with open(d / "train_uncontrolled_episode.csv", "w") as f:
        f.write("step,nusselt\n0,2.5\n1,2.75\n")
    got = env._load_uncontrolled_episode(0, EnvMode.TRAIN)
    assert list(got["step"]) == [0, 1] and list(got["nusselt"]) == [2.5, 2.75]
    assert env._load_uncontrolled_episode(1, env.mode) is None and env.get_uncontrolled_episode_metrics() is None
    from fluidgym_amd.envs.parallel_env import ParallelFluidEnv
    for name in ("compute_domain_statistics", "record_uncontrolled_episodes", "get_uncontrolled_episode_metrics"):
        with pytest.raises(NotImplementedError):
            getattr(ParallelFluidEnv, name)(object.__new__(ParallelFluidEnv))


def test_field_summary_abi():
    header = open(os.path.join(ROOT, "include", "fluidgym_hip.h")).read()
    assert re.search(r"\bint\s+fg_field_summary\s*\(", header)
    assert "fg_field_summary" in L.SIGNATURES and "fg_field_summary" in L.SIGNATURES_F64
    assert not "fg_field_summary".startswith(L._F64_ABSENT_PREFIXES)
    m = re.search(r"#define\s+FG_FIELD_SUMMARY_WORK_BYTES\s+(\d+)", header)
    assert m and int(m.group(1)) == L.FG_FIELD_SUMMARY_WORK_BYTES
    one = ctypes.c_void_p(64)          # never dereferenced: every call below fails its argument checks first
    for lib in (L.load(), L.load_f64()):
        f = lib.fg_field_summary
        bad = [
            (None, 1, 1, 8, 0, one, one, one, 0.0, 1.0, 8, one),          # null field
            (one, 1, 1, 0, 0, one, one, one, 0.0, 1.0, 8, one),           # n <= 0
            (one, 1, 2, 8, 2, one, one, one, 0.0, 1.0, 8, one),           # channel out of range
            (one, 1, 2, 8, -2, one, one, one, 0.0, 1.0, 8, one),
            (one, 1, 1, 8, 0, one, one, one, 0.0, 1.0, 0, one),           # nbins outside 1..4096
            (one, 1, 1, 8, 0, one, one, one, 0.0, 1.0, 4097, one),
            (one, 1, 1, 8, 0, one, one, one, 0.0, 0.0, 8, one),           # width <= 0 with a histogram
            (one, 1, 1, 8, 0, one, one, one, 0.0, -1.0, 8, one),
            (one, 1, 1, 8, 0, one, None, one, 0.0, 1.0, 8, None),         # moments asked for with a null output
            (one, 1, 1, 8, 0, None, None, None, 0.0, 1.0, 8, None),       # nothing asked for
        ]
        for args in bad:
            assert f(*args, None) == -1, args
            assert b"fg_field_summary" in lib.fg_last_error()
