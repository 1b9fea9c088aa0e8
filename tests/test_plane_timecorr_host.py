"""``HostPlaneTimeCorrelation``, the NumPy twin of ``fg_plane_timecorr``: the single-base mode against golden values of the
reference's ``TemporalTwoPointCorrelation_Online_torch``, the windowed mode against a brute-force evaluation over every (base, lag)
pair, the schedule's counts and times, merging, the integral time, the files and the argument checks."""
import glob
import os

import numpy as np
import pytest

from fluidgym_amd.simulation.plane_timecorr import FILE_META, FILE_RECORD, FILE_REFERENCE, HostPlaneTimeCorrelation, PlaneTimeCorrelation
from tests.plane_stats_ref import BOUND_GOLDEN
from tests.plane_timecorr_ref import brute_force, channel_stack, make_series

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_plane_timecorr.npz")
BOUND_BRUTE = 1e-12
VEL = ("u", "v", "w")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _feed(rec, series, times=None):
    for s, smp in enumerate(series):
        u, p, T = smp
        rec.update(u, p if "p" in rec.channels else None, T if "T" in rec.channels else None,
                   time=0.1 * s if times is None else times[s])
    return rec


def _golden_record(golden, lags=5):
    rec = HostPlaneTimeCorrelation(VEL, lags)
    for u, t in zip(golden["velocity"], golden["times"]):
        rec.update(u, time=t)
    return rec


def test_single_base_mode_equals_the_reference(golden):
    rec = _golden_record(golden)
    ref = rec.reference_arrays()
    err_c = float(np.abs(ref["steps_coefficients"] - golden["steps_coefficients"]).max())
    err_r = float(np.abs(ref["base_rms"] - golden["base_rms"]).max())
    print(f"coefficients {err_c:.2e} base_rms {err_r:.2e}")
    assert err_c <= BOUND_GOLDEN and err_r <= BOUND_GOLDEN
    assert np.abs(ref["base_fluctuations"] - golden["base_fluctuations"]).max() <= BOUND_GOLDEN
    assert np.array_equal(ref["steps_time"], golden["steps_time"])
    assert rec.count.tolist() == [1.0] * 5 and rec.full
    for k, c in enumerate(VEL):                               # one base: the coefficient is also the ratio of the sums
        assert np.abs(rec.coefficient(c) - np.moveaxis(golden["steps_coefficients"][:, :, k], 0, -1)).max() <= BOUND_GOLDEN
        assert np.abs(rec.correlation(c) - rec.coefficient(c)).max() <= 1e-12
        assert np.abs(rec.normalized(c)[..., 0] - 1.0).max() == 0.0


def test_saved_files_have_the_reference_layout(golden, tmp_path):
    rec = _golden_record(golden)
    rec.save(tmp_path)
    assert sorted(os.path.basename(f) for f in glob.glob(str(tmp_path / "*"))) == sorted([FILE_RECORD, FILE_META, FILE_REFERENCE])
    with np.load(tmp_path / FILE_REFERENCE) as z:
        assert sorted(z.files) == sorted(list(golden["keys_temporal"]) + ["steps_time_envs"])
        assert z["base_fluctuations"].shape == (2, 3, 4, 3, 10) and z["base_rms"].shape == (2, 3, 3)
        assert z["steps_coefficients"].shape == (5, 2, 3, 3) and z["steps_time"].shape == (5,) and z["steps_time_envs"].shape == (5, 2)
        for k in ("base_fluctuations", "base_rms", "steps_coefficients", "steps_time"):
            assert z[k].shape == golden[k].shape and z[k].dtype == golden[k].dtype
    back = HostPlaneTimeCorrelation.load(tmp_path)
    assert back._state().tobytes() == rec._state().tobytes() and back.count.tolist() == rec.count.tolist()
    assert np.array_equal(back.lag_time(), rec.lag_time())
    # a windowed record, or one with the pressure, has no reference file
    series = make_series((1, 2, 3, 4), VEL + ("p",), 3, dtype=np.float64)
    other = tmp_path / "windowed"
    _feed(HostPlaneTimeCorrelation(VEL + ("p",), 2, 1), series).save(other)
    assert not os.path.exists(other / FILE_REFERENCE) and os.path.exists(other / FILE_RECORD)


def test_the_references_own_load_reads_the_saved_file(golden, tmp_path):
    ref_root = os.environ.get("FLUIDGYM_REFERENCE", "")
    if not os.path.exists(os.path.join(ref_root, "simulation", "pict", "data", "online_statistics.py")):
        pytest.skip("the reference is not importable here (FLUIDGYM_REFERENCE=<reference>/src/fluidgym)")
    import sys
    import torch

    sys.path.insert(0, os.path.join(os.path.dirname(GOLDEN)))
    from make_golden_plane_stats import load_reference_statistics

    S = load_reference_statistics(ref_root)
    _golden_record(golden).save(tmp_path)
    corr = S.TemporalTwoPointCorrelation_Online_torch([2, 4])
    corr.load(str(tmp_path / FILE_REFERENCE), dtype=torch.float64)
    assert np.abs(corr.base_rms.numpy() - golden["base_rms"]).max() <= BOUND_GOLDEN
    assert np.abs(np.asarray(corr.steps_coefficients) - golden["steps_coefficients"]).max() <= BOUND_GOLDEN


@pytest.mark.parametrize("lags,stride,samples", [(4, 2, 7), (3, 1, 7), (2, 2, 6), (5, None, 7)])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["fp32", "fp64"])
def test_windowed_mode_equals_the_brute_force_over_every_pair(lags, stride, samples, dtype):
    channels = ("u", "v", "w", "p")
    series = make_series((2, 3, 4, 6), channels, samples, seed=3, dtype=dtype)
    times = [np.array([0.1 * s, 0.25 * s + 0.01 * s * s]) for s in range(samples)]         # per env, not uniform
    rec = _feed(HostPlaneTimeCorrelation(channels, lags, stride), series, times)
    acc, count, time_sum = brute_force([channel_stack(s, channels) for s in series], times, lags, stride, dtype)
    assert rec.count.tolist() == count.tolist()
    assert np.abs(rec.time_sum - time_sum).max() <= 1e-14
    assert np.allclose(rec.lag_time(), time_sum / count, rtol=0, atol=1e-14)
    for k, c in enumerate(channels):
        want_coef = acc[:, :, k, :, 0] / count
        want_corr = acc[:, :, k, :, 1] / np.sqrt(acc[:, :, k, :, 2] * acc[:, :, k, :, 3])
        e1, e2 = float(np.abs(rec.coefficient(c) - want_coef).max()), float(np.abs(rec.correlation(c) - want_corr).max())
        print(f"lags {lags} stride {stride} {c}: coefficient {e1:.2e} correlation {e2:.2e}")
        assert e1 <= BOUND_BRUTE and e2 <= BOUND_BRUTE
    if stride is None:
        assert rec.full and rec.samples == samples and len(rec.times) == lags       # two samples were dropped
    else:
        assert not rec.full and len(rec.times) == samples


def test_the_schedule_reuses_its_slots():
    rec = HostPlaneTimeCorrelation(VEL, 4, 2)
    assert rec.n_slots == 2
    tables = []
    for s, smp in enumerate(make_series((1, 2, 2, 4), VEL, 7, dtype=np.float64)):
        tables.append(rec.slot_lags(s))
        rec.update(smp[0], time=float(s))
    assert tables == [[0, -1], [1, -1], [2, 0], [3, 1], [0, 2], [1, 3], [2, 0]]
    assert rec.count.tolist() == [4.0, 3.0, 3.0, 2.0]
    assert HostPlaneTimeCorrelation(VEL, 2, 2).n_slots == 1 and HostPlaneTimeCorrelation(VEL, 8, 1).n_slots == 8
    one = HostPlaneTimeCorrelation(VEL, 3)
    assert [one.slot_lags(s) for s in range(4)] == [[0], [1], [2], [-1]]


def test_merge_adds_two_records_and_pooled_sums_the_envs():
    channels, lags, stride = VEL, 3, 1
    first = make_series((2, 2, 3, 5), channels, 5, seed=5, dtype=np.float64)
    second = make_series((2, 2, 3, 5), channels, 4, seed=6, dtype=np.float64)
    a, b = (_feed(HostPlaneTimeCorrelation(channels, lags, stride), s) for s in (first, second))
    parts = [brute_force([channel_stack(s, channels) for s in ser], [np.full(2, 0.1 * i) for i in range(len(ser))], lags, stride)
             for ser in (first, second)]
    acc, count = parts[0][0] + parts[1][0], parts[0][1] + parts[1][1]
    a.merge(b)
    assert a.count.tolist() == count.tolist()
    assert np.abs(a.coefficient("v") - acc[:, :, 1, :, 0] / count).max() <= BOUND_BRUTE
    assert np.abs(a.lag_time() - 0.1 * np.arange(lags)).max() <= 1e-14
    pooled = a.pooled()
    assert pooled.count.tolist() == (2 * count).tolist() and pooled._state().shape[0] == 1
    assert np.abs(pooled.coefficient("v") - acc[:, :, 1, :, 0].sum(axis=0, keepdims=True) / (2 * count)).max() <= BOUND_BRUTE
    want = acc[:, :, 0, :, 1].sum(axis=0) / np.sqrt(acc[:, :, 0, :, 2].sum(axis=0) * acc[:, :, 0, :, 3].sum(axis=0))
    assert np.abs(pooled.correlation("u")[0] - want).max() <= BOUND_BRUTE
    assert np.abs(pooled.lag_time() - 0.1 * np.arange(lags)).max() <= 1e-14
    with pytest.raises(ValueError, match="same channels, lags and stride"):
        a.merge(HostPlaneTimeCorrelation(channels, lags, 2))
    with pytest.raises(ValueError, match="changed between updates"):
        a.update(make_series((3, 2, 3, 5), channels, 1, dtype=np.float64)[0][0])


def test_integral_time_of_an_exponential_and_of_a_crossing():
    # exp(-t / T) with T = 0.5 over 200 lags of 0.02: the trapezoid differs from T by its own error, T (dt / T)^2 / 12 = 7e-5, and by
    # the truncated tail, T exp(-8) = 2e-4
    long = HostPlaneTimeCorrelation(("u",), 200)
    t = 0.02 * np.arange(200)
    r = np.exp(-t / 0.5)
    acc = np.zeros((1, 1, 1, 200, 4))
    acc[0, 0, 0, :, 1], acc[0, 0, 0, :, 2], acc[0, 0, 0, :, 3] = r, 1.0, 1.0
    long._set_state(acc)
    long.count, long.time_sum = np.ones(200), t[None].copy()
    got = long.integral_time("u")[0, 0]
    assert abs(got - float(np.sum(0.5 * (r[1:] + r[:-1]) * 0.02))) <= 1e-13
    assert abs(got - 0.5) <= 3e-4
    rec = HostPlaneTimeCorrelation(("u",), 6, 1)
    t = 0.2 * np.arange(6)
    acc = np.ones((1, 1, 1, 6, 4))
    rec.count, rec.time_sum = np.ones(6), t[None].copy()
    acc[0, 0, 0, :, 1] = [1.0, 0.5, -0.5, 0.7, 0.7, 0.7]                            # crosses zero half way between lags 1 and 2
    rec._set_state(acc)
    assert abs(rec.integral_time("u")[0, 0] - (0.5 * 1.5 * 0.2 + 0.5 * 0.5 * 0.1)) <= 1e-15
    rec.set_wall_units([-0.5, 0.5], 0.01, 0.05)
    assert np.allclose(rec.lag_ETT(), t[None] * 0.05) and np.allclose(rec.lag_t_wall(), t[None] * 0.05 ** 2 / 0.01)
    assert np.allclose(rec.to_wall_pos([-0.5]), 0.5 * 0.05 / 0.01)


def test_argument_checks():
    with pytest.raises(ValueError, match="more than the 8"):
        HostPlaneTimeCorrelation(VEL, 9, 1)
    with pytest.raises(ValueError, match="more than the 8"):
        PlaneTimeCorrelation(VEL, 17, 2)
    assert HostPlaneTimeCorrelation(VEL, 16, 2).n_slots == 8
    for bad in ((), ("u", "u"), ("u", "q")):
        with pytest.raises(ValueError, match="channels must be"):
            HostPlaneTimeCorrelation(bad, 2)
    with pytest.raises(ValueError, match="lags must be at least 1"):
        HostPlaneTimeCorrelation(VEL, 0)
    with pytest.raises(ValueError, match="stride must be"):
        HostPlaneTimeCorrelation(VEL, 2, 0)
    with pytest.raises(RuntimeError, match="no sample recorded yet"):
        HostPlaneTimeCorrelation(VEL, 2).coefficient("u")
    with pytest.raises(ValueError, match="do not fit"):
        HostPlaneTimeCorrelation(VEL, 2).update(np.zeros((1, 2, 4, 4)))
    with pytest.raises(ValueError, match="tensors on the GPU"):
        PlaneTimeCorrelation(VEL, 2).update(np.zeros((1, 3, 2, 4, 4), np.float32))


@pytest.mark.parametrize("lib_name", ["fp32", "fp64"])
def test_the_entry_point_refuses_bad_tables_before_it_launches(lib_name):
    """The argument checks of ``fg_plane_timecorr`` return before anything touches the device: the pointers here are never read."""
    import ctypes

    from fluidgym_amd import _lib as L

    lib = L.load() if lib_name == "fp32" else L.load_f64()
    fake = ctypes.c_void_p(4096)

    def call(K=3, batch=2, nz=4, ny=3, nx=8, lags=4, table=(0, -1), stride=4 * 3 * 8 * 3, base=fake):
        ptrs = (ctypes.c_void_p * 5)(*([4096] * 5))
        strides = (ctypes.c_int64 * 5)(*([stride] * 5))
        slots = (ctypes.c_int32 * max(len(table), 1))(*table)
        rc = lib.fg_plane_timecorr(ptrs, strides, K, batch, nz, ny, nx, lags, len(table), slots, base, fake, fake, None)
        return rc, lib.fg_last_error().decode()

    for kw, text in ((dict(table=()), "n_slots must be 1..8"), (dict(table=(-1,) * 9), "n_slots must be 1..8"),
                     (dict(table=(-2, 0)), "outside [-1, lags)"), (dict(table=(0, 4)), "outside [-1, lags)"),
                     (dict(table=(1, 2, 1)), "two slots with the same lag"), (dict(table=(0, 0)), "two slots with the same lag"),
                     (dict(K=0), "K must be 1..5"), (dict(K=6), "K must be 1..5"), (dict(lags=0), "lags must be positive"),
                     (dict(nx=0), "must be positive"), (dict(stride=95), "batch stride smaller"), (dict(base=None), "null base")):
        rc, msg = call(**kw)
        assert rc == -1 and text in msg, (kw, rc, msg)                       # FG_ERR_INVALID_ARG
    assert call(table=(-1, -1))[0] == 0                                       # every slot idle: nothing to record, nothing launched
