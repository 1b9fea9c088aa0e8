"""``HostSignalSpectra``, the NumPy twin of ``fg_signal_spectra``, against ``scipy.signal.welch`` / ``csd``; per-env restarts; the
record's accessors, merging and files; the argument checks of the spec and of the entry point; the env wiring on a stub.  No GPU."""
import ctypes

import numpy as np
import pytest
import torch

from fluidgym_amd.envs.signal_spectra import SignalSpectraMixin
from fluidgym_amd.envs.step_hooks import HOOK_ORDER, StepHooksMixin
from fluidgym_amd.simulation.signal_spectra import (HostSignalSpectra, SignalSpectra, SignalSpectraRecord, check_extents,
                                                    max_segment)
from tests.signal_spectra_ref import DETRENDS, n_segments, rel_max, scipy_welch, three_signals

BOUND_SCIPY = 1e-13
NAMES = ("a", "b", "c")
PAIRS = (("a", "b"), ("b", "c"))
DT = 0.05


def _windows(L):
    return {"hann": "hann", "boxcar": np.ones(L)}


def _feed(rec, series):
    for smp in series:
        rec.update(smp)
    return rec


@pytest.mark.parametrize("detrend", DETRENDS)
@pytest.mark.parametrize("overlap", ["0", "L/2", "3L/4"])
@pytest.mark.parametrize("L", [16, 32, 64, 1024])
def test_the_twin_equals_scipy_welch_and_csd(L, overlap, detrend):
    noverlap = {"0": 0, "L/2": L // 2, "3L/4": 3 * L // 4}[overlap]
    x = three_signals(L, seed=L)
    for wname, window in _windows(L).items():
        rec = _feed(HostSignalSpectra(NAMES, L, noverlap, window, detrend, PAIRS, DT), x[:, None, :])
        assert rec.segments.tolist() == [n_segments(len(x), L, noverlap)]
        for s, name in enumerate(NAMES):
            err = rel_max(rec.psd(name)[0], scipy_welch(x[:, s], None, L, noverlap, window, detrend, DT))
            print(f"L {L} noverlap {noverlap} {detrend} {wname} psd {name}: {err:.2e}")
            assert err <= BOUND_SCIPY
        for a, b in PAIRS:
            want = scipy_welch(x[:, NAMES.index(a)], x[:, NAMES.index(b)], L, noverlap, window, detrend, DT)
            err = rel_max(rec.csd(a, b)[0], want)
            print(f"L {L} noverlap {noverlap} {detrend} {wname} csd {a} {b}: {err:.2e}")
            assert err <= BOUND_SCIPY
            assert rel_max(rec.csd(b, a)[0], np.conj(want)) <= BOUND_SCIPY
    from scipy.signal import get_window

    assert np.array_equal(rec.frequencies(), np.fft.rfftfreq(L, DT))
    assert np.array_equal(HostSignalSpectra(NAMES, L).window, get_window("hann", L)) and HostSignalSpectra(NAMES, L).noverlap == L // 2


@pytest.mark.parametrize("noverlap", [0, 8, 12])
def test_a_restart_drops_the_open_segment_of_the_chosen_env_only(noverlap):
    L, cut = 16, 2 * 16 + 3
    x = three_signals(L, seed=3)
    rec = HostSignalSpectra(NAMES, L, noverlap, "hann", "linear", PAIRS, DT)
    for i, smp in enumerate(x):
        if i == cut:
            rec.restart([1])
        rec.update(np.stack([smp, smp]))
    n_all, n1, n2 = (n_segments(n, L, noverlap) for n in (len(x), cut, len(x) - cut))
    assert rec.segments.tolist() == [n_all, n1 + n2]
    assert (n_all, n1, n2) == {0: (5, 2, 3), 8: (9, 3, 5), 12: (18, 5, 10)}[noverlap]      # 87 samples; 35 and 52: by hand
    for s, name in enumerate(NAMES):
        whole = scipy_welch(x[:, s], None, L, noverlap, "hann", "linear", DT)
        parts = [scipy_welch(piece[:, s], None, L, noverlap, "hann", "linear", DT) for piece in (x[:cut], x[cut:])]
        assert rel_max(rec.psd(name)[0], whole) <= BOUND_SCIPY
        assert rel_max(rec.psd(name)[1], (n1 * parts[0] + n2 * parts[1]) / (n1 + n2)) <= BOUND_SCIPY
    a, b = x[:, 0], x[:, 1]
    parts = [scipy_welch(a[sl], b[sl], L, noverlap, "hann", "linear", DT) for sl in (slice(0, cut), slice(cut, None))]
    assert rel_max(rec.csd("a", "b")[1], (n1 * parts[0] + n2 * parts[1]) / (n1 + n2)) <= BOUND_SCIPY
    # the last segment of env 0 alone
    end = L + (n_all - 1) * (L - noverlap)
    assert rel_max(rec.latest("c")[0], scipy_welch(x[end - L:end, 2], None, L, 0, "hann", "linear", DT)) <= BOUND_SCIPY


def test_the_ring_is_rounded_to_the_dtype_of_the_signals():
    L = 16
    x = three_signals(L, seed=5)
    rec32 = _feed(HostSignalSpectra(NAMES, L), x[:, None, :].astype(np.float32))
    rec64 = _feed(HostSignalSpectra(NAMES, L), x[:, None, :].astype(np.float32).astype(np.float64))
    assert rec32._ring.dtype == np.float32 and rec64._ring.dtype == np.float64
    err = rel_max(rec32.psd("a"), rec64.psd("a"))
    assert 0.0 < err < 1e-6                                    # the detrended, windowed segment is rounded once more
    with pytest.raises(ValueError, match="batch size changed"):
        rec32.update(np.zeros((2, 3), np.float32))
    with pytest.raises(ValueError, match="the sources hold 2 signals"):
        rec32.update(np.zeros((1, 2), np.float32))


def test_merge_pooled_and_the_files(tmp_path):
    L = 32
    x, y = three_signals(L, seed=7), three_signals(L, seed=8)
    two = np.stack([x, y], axis=1)                              # two envs with their own series
    a = _feed(HostSignalSpectra(NAMES, L, 8, "hann", "constant", PAIRS, DT), two)
    b = _feed(HostSignalSpectra(NAMES, L, 8, "hann", "constant", PAIRS, DT), two[::-1].copy())
    pa, pb, na = a.psd("a").copy(), b.psd("a").copy(), a.segments.copy()
    merged = a.record().merge(b)
    assert merged.segments.tolist() == (2 * na).tolist()
    assert rel_max(merged.psd("a"), 0.5 * (pa + pb)) <= 1e-15
    assert np.array_equal(merged.latest("a"), b.latest("a"))
    pooled = a.pooled()
    assert pooled.segments.tolist() == [int(na.sum())] and pooled.psd("b").shape == (1, L // 2 + 1)
    assert rel_max(pooled.psd("b")[0], a.psd("b").mean(axis=0)) <= 1e-15
    assert rel_max(pooled.csd("a", "b")[0], a.csd("a", "b").mean(axis=0)) <= 1e-15
    with pytest.raises(ValueError, match="same names, segment"):
        a.merge(HostSignalSpectra(NAMES, L, 16, "hann", "constant", PAIRS, DT))
    with pytest.raises(ValueError, match="same names, segment"):
        a.merge(_feed(HostSignalSpectra(NAMES, L, 8, np.ones(L), "constant", PAIRS, DT), two))
    with pytest.raises(RuntimeError, match="no sample yet"):
        HostSignalSpectra(NAMES, L, 8, "hann", "constant", PAIRS, DT).merge(a)
    a.save(tmp_path / "spectra")
    assert sorted(p.name for p in tmp_path.iterdir()) == ["spectra.json", "spectra.npz"]
    back = SignalSpectraRecord.load(tmp_path / "spectra.npz")
    assert back.spec() == a.spec() and back.names == NAMES and back.pairs == PAIRS
    for got, want in zip(back._state(), a._state()):
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes()
    assert np.array_equal(back.psd("c"), a.psd("c")) and np.array_equal(back.window, a.window)


def test_coherence_phase_peak_and_envs_without_a_segment():
    L, n = 64, 5 * 64 + 7
    t = np.arange(n) * DT
    f0 = 5.2 / (L * DT)                                         # a fifth of a bin above bin 5
    sine = np.sin(2.0 * np.pi * f0 * t)
    lag = np.sin(2.0 * np.pi * f0 * t - 0.6)
    rec = HostSignalSpectra(("s", "lag"), L, L // 2, "hann", "constant", (("s", "s"), ("s", "lag")), DT)
    short = 40                                                  # env 1 sees fewer samples than a segment: restarted near the end
    for i in range(n):
        if i == n - short:
            rec.restart([1])
        rec.update(np.array([[sine[i], lag[i]]] * 2))
    assert rec.segments.tolist() == [n_segments(n, L, L // 2), n_segments(n - short, L, L // 2)]
    assert np.array_equal(rec.coherence("s", "s")[0], np.ones(L // 2 + 1)) and np.all(rec.csd("s", "s")[0].imag == 0.0)
    assert np.array_equal(rec.csd("s", "s")[0].real, rec.psd("s")[0])
    df = 1.0 / (L * DT)
    peak = rec.peak_frequency("s")
    print(f"peak {peak[0] / df:.4f} bins, true {f0 / df:.4f}")
    assert abs(peak[0] - f0) <= 0.25 * df
    assert abs(rec.peak_frequency("s", band=(3 * df, 8 * df))[0] - f0) <= 0.25 * df
    assert abs(rec.strouhal("s", 2.0, 4.0)[0] - 0.5 * peak[0]) <= 1e-15
    k = 5
    assert abs(rec.phase("s", "lag")[0, k] + 0.6) <= 1e-2 and rec.coherence("s", "lag")[0, k] > 0.999
    with pytest.raises(ValueError, match="holds no bin"):
        rec.peak_frequency("s", band=(1e3, 2e3))
    with pytest.raises(KeyError, match="is not recorded"):
        _feed(HostSignalSpectra(("s", "lag"), 16), np.zeros((1, 1, 2))).csd("s", "lag")      # an unlisted pair
    with pytest.raises(KeyError, match="no signal"):
        rec.psd("nope")
    # an env without a segment: NaN, and no warning
    fresh = HostSignalSpectra(("s",), 16)
    for i in range(20):
        fresh.update(np.array([sine[i], 0.0 if i < 10 else sine[i]]))
        if i == 9:
            fresh.restart([1])
    assert fresh.segments.tolist() == [1, 0]
    with np.errstate(all="raise"):
        assert np.isfinite(fresh.psd("s")[0]).all() and np.isnan(fresh.psd("s")[1]).all()
        assert np.isnan(fresh.latest("s")[1]).all() and np.isnan(fresh.peak_frequency("s")[1]) and np.isfinite(fresh.peak_frequency("s")[0])
        assert np.isnan(fresh.coherence("s", "s")[1]).all()


def test_a_non_finite_sample_marks_its_signal_and_its_pairs_only():
    L = 16
    x = three_signals(L, seed=11)[:, None, :].repeat(2, axis=1)
    bad = x.copy()
    bad[20, 0, 2] = np.nan
    clean = _feed(HostSignalSpectra(NAMES, L, 8, "hann", "constant", PAIRS), x)
    rec = _feed(HostSignalSpectra(NAMES, L, 8, "hann", "constant", PAIRS), bad)
    assert np.isnan(rec.psd("c")[0]).all() and np.isnan(rec.csd("b", "c")[0]).all()
    for name in ("a", "b"):
        assert rec.psd(name).tobytes() == clean.psd(name).tobytes()
    assert rec.csd("a", "b").tobytes() == clean.csd("a", "b").tobytes()
    assert rec.psd("c")[1].tobytes() == clean.psd("c")[1].tobytes() and rec.segments.tolist() == clean.segments.tolist()


def test_the_spec_refusals():
    with pytest.raises(ValueError, match="distinct signal names"):
        HostSignalSpectra(())
    with pytest.raises(ValueError, match="distinct signal names"):
        HostSignalSpectra(("a", "a"))
    with pytest.raises(ValueError, match="distinct signal names"):
        SignalSpectra([f"s{i}" for i in range(65)])
    for seg in (8, 24, 100):
        with pytest.raises(ValueError, match="power of two, at least 16"):
            HostSignalSpectra(NAMES, seg)
    with pytest.raises(ValueError, match="does not fit in 160 KB"):
        SignalSpectra(NAMES, 8192)
    with pytest.raises(ValueError, match="at most 2048"):
        check_extents(4096, torch.float64)
    check_extents(4096, torch.float32)
    assert max_segment(torch.float32) == 4096 and max_segment(np.float64) == 2048
    with pytest.raises(ValueError, match="at most 2048"):                      # refused at the first sample of fp64 signals at the latest
        HostSignalSpectra(("a",), 4096).update(np.zeros(1))
    for nov in (-1, 16, 17):
        with pytest.raises(ValueError, match=r"noverlap must lie in \[0, segment = 16\)"):
            HostSignalSpectra(NAMES, 16, nov)
    with pytest.raises(ValueError, match="detrend must be one of"):
        HostSignalSpectra(NAMES, 16, detrend="quadratic")
    with pytest.raises(ValueError, match=r"array \[16\]"):
        HostSignalSpectra(NAMES, 16, window=np.ones(15))
    with pytest.raises(ValueError, match="finite and not all zero"):
        HostSignalSpectra(NAMES, 16, window=np.zeros(16))
    with pytest.raises(ValueError, match="names a signal that is not recorded"):
        HostSignalSpectra(NAMES, 16, pairs=[("a", "q")])
    with pytest.raises(ValueError, match="at most 64 distinct"):
        HostSignalSpectra(NAMES, 16, pairs=[("a", "b"), ("a", "b")])
    with pytest.raises(ValueError, match="dt, the sample interval, must be positive"):
        HostSignalSpectra(NAMES, 16, dt=0.0)
    with pytest.raises(RuntimeError, match="no sample recorded yet"):
        HostSignalSpectra(NAMES, 16).psd("a")
    with pytest.raises(RuntimeError, match="no sample recorded yet"):
        SignalSpectra(NAMES, 16).segments
    with pytest.raises(ValueError, match="1..8 sources"):
        HostSignalSpectra(NAMES, 16).update()
    with pytest.raises(ValueError, match=r"\[B\] or \[B, n\]"):
        HostSignalSpectra(NAMES, 16).update(np.zeros((2, 3, 1)))
    with pytest.raises(ValueError, match="tensors on the GPU"):
        SignalSpectra(NAMES, 16).update(np.zeros((2, 3), np.float32))


def test_the_entry_point_is_declared_and_typed_for_both_libraries():
    import os
    import re

    from fluidgym_amd import _lib as L

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fluidgym_hip.h")).read()
    decl = re.search(r"\bint fg_signal_spectra\(([^;]*)\);", header)
    assert decl and len(decl.group(1).split(",")) == 18
    for table in (L.SIGNATURES, L.SIGNATURES_F64):
        res, args = table["fg_signal_spectra"]
        assert res is ctypes.c_int and len(args) == 18


@pytest.mark.parametrize("lib_name", ["fp32", "fp64"])
def test_the_entry_point_refuses_bad_arguments_before_it_launches(lib_name):
    """The argument checks of ``fg_signal_spectra`` return before anything touches the device: the pointers here are never read."""
    from fluidgym_amd import _lib as L

    lib = L.load() if lib_name == "fp32" else L.load_f64()
    fake = ctypes.c_void_p(4096)

    def call(widths=(2, 3), batch=3, seg=16, noverlap=8, detrend=1, pairs=((0, 1), (1, 4)), strides=None, window=fake, ring=fake,
             fill=fake, power=fake, cross=fake, segments=fake, n_sources=None, n_pairs=None, src=4096):
        n = max(len(widths), 1)
        ptrs = (ctypes.c_void_p * n)(*([src] * n))
        st = (ctypes.c_int64 * n)(*(strides or widths or (0,)))
        wid = (ctypes.c_int32 * n)(*(widths or (0,)))
        flat = [i for p in pairs for i in p] or [0]
        tab = (ctypes.c_int32 * len(flat))(*flat)
        rc = lib.fg_signal_spectra(ptrs, st, wid, len(widths) if n_sources is None else n_sources, batch, seg, noverlap, detrend, window,
                                   tab, len(pairs) if n_pairs is None else n_pairs, ring, fill, power, cross, segments, None, None)
        return rc, lib.fg_last_error().decode()

    invalid, unsupported = -1, L.FG_ERR_UNSUPPORTED
    for kw, text in ((dict(n_sources=0), "n_sources must be 1..8"), (dict(widths=(1,) * 9), "n_sources must be 1..8"),
                     (dict(widths=(0, 3)), "widths must be positive"), (dict(widths=(32, 32, 1)), "sum to 1..64"),
                     (dict(widths=(65,)), "sum to 1..64"), (dict(strides=(1, 3)), "batch stride smaller"),
                     (dict(n_pairs=65), "n_pairs must be 0..64"), (dict(n_pairs=-1), "n_pairs must be 0..64"),
                     (dict(pairs=((0, 5),)), "pair index outside [0, S)"), (dict(pairs=((-1, 0),)), "pair index outside [0, S)"),
                     (dict(noverlap=16), "noverlap must lie in [0, segment)"), (dict(noverlap=-1), "noverlap must lie in [0, segment)"),
                     (dict(detrend=3), "detrend must be 0"), (dict(detrend=-1), "detrend must be 0"),
                     (dict(batch=0), "batch must be positive"), (dict(src=None), "null source pointer"),
                     (dict(window=None), "null window"), (dict(ring=None), "null window"), (dict(fill=None), "null window"),
                     (dict(power=None), "null window"), (dict(segments=None), "null window"),
                     (dict(cross=None), "null pair table or cross")):
        rc, msg = call(**kw)
        assert rc == invalid and text in msg, (kw, rc, msg)                   # FG_ERR_INVALID_ARG
    top = 4096 if lib_name == "fp32" else 2048
    for kw, text in ((dict(seg=8, noverlap=4), "power of two, at least 16"), (dict(seg=48), "power of two, at least 16"),
                     (dict(seg=2 * top), f"segment <= {top}"), (dict(seg=1 << 30), f"segment <= {top}")):
        rc, msg = call(**kw)
        assert rc == unsupported and text in msg, (kw, rc, msg)


# ---- the env wiring on a stub: the calls FluidEnv makes, without a simulation (StubEnv of test_step_hooks_host.py)
class Target:
    def __init__(self):
        self.runs, self.reseeds = 0, []

    def run(self):
        self.runs += 1

    def reseed(self, envs=None):
        self.reseeds.append(envs)


class StubEnv(SignalSpectraMixin, StepHooksMixin):
    _domain, _dtype, _num_envs = object(), torch.float64, 2

    def __init__(self):
        self.clock, self.calls = 0, 0

    def _signal_sample_time(self):
        return 0.25

    def _make_signal_recorder(self, *spec):
        return HostSignalSpectra(*spec)

    def value(self):                                            # used unbound: a callable(env)
        self.calls += 1
        return torch.tensor([[np.sin(0.9 * self.clock), 1.0], [np.cos(0.4 * self.clock), 2.0]], dtype=torch.float64)

    def step(self, n=1):
        for _ in range(n):
            self.clock += 1
            self._after_sim_step()

    def reset(self):
        self._reseed_hooks()

    def reset_envs(self, envs):
        self._reseed_hooks(envs)

    def set_state(self, state):
        self._load_hooks_state(state)

    def close(self):
        self._step_hooks = {}
        self._signal_spectra_active = None


def test_the_mixin_samples_every_nth_step_after_the_hooks_and_restarts_with_the_env():
    assert HOOK_ORDER == ("flow_stats", "flow_spectra", "flow_budgets", "flow_timecorr", "flow_hist", "field_stats", "tracers",
                          "mesh_tracers")
    env, hook = StubEnv(), Target()
    assert env.signal_spectra is None
    with pytest.raises(RuntimeError, match="no signal spectra are being recorded"):
        env.stop_signal_spectra()
    env._start_hook("tracers", hook, 1, hook.run, reseed=hook.reseed, state_key="tracers")
    env.step(3)                                                 # without a recorder the hooks run as they did
    assert hook.runs == 3 and env.calls == 0
    rec = env.start_signal_spectra({"q": StubEnv.value}, segment=16, noverlap=8, pairs=[("q[0]", "q[1]")], every=2)
    assert env.signal_spectra is rec and rec.names == ("q[0]", "q[1]") and rec.dt == 0.5 and env.calls == 1
    assert list(env._step_hooks) == ["tracers"]                 # no ninth hook
    env.step(7)
    assert env.calls == 1 + 3 and rec._fill.tolist() == [3, 3] and hook.runs == 10
    env.step(1)
    assert rec._fill.tolist() == [4, 4]
    env.reset_envs([1])
    assert rec._fill.tolist() == [4, 0] and hook.reseeds == [[1]] and env._signal_spectra_active.tick == 8
    env.step(40)
    assert rec._fill.tolist() == [24, 20] and rec.segments.tolist() == [2, 1]
    env.reset()
    assert rec._fill.tolist() == [0, 0] and rec.segments.tolist() == [2, 1] and env._signal_spectra_active.tick == 0
    env.step(4)
    assert rec._fill.tolist() == [2, 2]
    env.set_state({})
    assert rec._fill.tolist() == [0, 0] and rec.segments.tolist() == [2, 1]
    with pytest.raises(RuntimeError, match="holds a tracer cloud but none is active"):      # the hooks' own refusals pass through
        StubEnv().set_state({"tracers": {}})
    assert env.stop_signal_spectra() is rec and env.signal_spectra is None
    calls = env.calls
    env.step(4)
    assert env.calls == calls and rec._fill.tolist() == [0, 0] and hook.runs == 59
    # a fresh recorder replaces a live one; close drops it
    first = env.start_signal_spectra([("q", StubEnv.value)], segment=16)
    second = env.start_signal_spectra([("q", StubEnv.value)], segment=32)
    assert env.signal_spectra is second and first is not second and second.noverlap == 16
    env.close()
    assert env.signal_spectra is None


def test_start_refusals_on_the_stub():
    env = StubEnv()
    with pytest.raises(ValueError, match="every must be at least 1"):
        env.start_signal_spectra({"q": StubEnv.value}, every=0)
    with pytest.raises(ValueError, match="power of two"):
        env.start_signal_spectra({"q": StubEnv.value}, segment=100)
    with pytest.raises(ValueError, match="at most 2048"):                      # the stub's dtype is float64
        env.start_signal_spectra({"q": StubEnv.value}, segment=4096)
    with pytest.raises(ValueError, match="no built-in signal 'lift'"):
        env.start_signal_spectra(["lift"])
    with pytest.raises(ValueError, match="1..8 sources"):
        env.start_signal_spectra(())
    with pytest.raises(ValueError, match="1..8 sources"):
        env.start_signal_spectra([(f"q{i}", StubEnv.value) for i in range(9)])
    with pytest.raises(ValueError, match=r"must return a tensor \[B\] or \[B, n\] with B = 2"):
        env.start_signal_spectra({"q": lambda e: torch.zeros(3)})
    with pytest.raises(ValueError, match="not recorded"):
        env.start_signal_spectra({"q": StubEnv.value}, segment=16, pairs=[("q", "q")])
    assert env.signal_spectra is None
    blank = StubEnv()
    blank._domain = None
    with pytest.raises(RuntimeError, match="reset\\(\\) the env first"):
        blank.start_signal_spectra({"q": StubEnv.value})


def test_parallel_env_refuses_by_name():
    from fluidgym_amd.envs.parallel_env import ParallelFluidEnv

    env = object.__new__(ParallelFluidEnv)
    for name, call in (("start_signal_spectra", lambda: env.start_signal_spectra(["lift"], segment=16)),
                       ("stop_signal_spectra", lambda: env.stop_signal_spectra()), ("signal_spectra", lambda: env.signal_spectra)):
        with pytest.raises(NotImplementedError, match=f"{name} is not implemented for ParallelFluidEnv"):
            call()
