"""``fg_signal_spectra`` / ``SignalSpectra`` on the GPU, both libraries: the kernel against the NumPy twin with the envs out of phase,
independence of an env from the rest of the batch, what a non-finite sample does, and the env layer on a multi-block and a
single-block env.

``B = 3``, ``S = 5`` from two sources of widths 2 and 3 (an odd ``S``), pairs ``(0, 1)``, ``(1, 4)``, ``(2, 2)``; ``L`` = 16 (radix 4
alone), 32 (radix 4 and the radix-2 tail), 64 (one butterfly per lane) and once 1024 (several per lane); ``5 L + 7`` samples, env 1
restarted once in the middle of a segment.

Bounds.  fp64 library: ``1e-12`` of the largest bin of the signal (cross: of the pair).  fp32 library: 16 times the error, in the same
measure and on the same segments, of ``scipy.fft.rfft`` run in single precision against the fp64 twin (16: radix 4 against
pocketfft's ordering, a full complex transform against a real one)."""
import numpy as np
import pytest
import torch

import fluidgym_amd
from fluidgym_amd.simulation.signal_spectra import DETRENDS, HostSignalSpectra, SignalSpectra
from tests.signal_spectra_ref import batch_series

pytestmark = pytest.mark.gpu

DTYPES = {"fp32": np.float32, "fp64": np.float64}
WIDTHS = (2, 3)
NAMES = ("s0", "s1", "s2", "s3", "s4")
PAIRS = (("s0", "s1"), ("s1", "s4"), ("s2", "s2"))
BOUND_FP64 = 1e-12
FP32_FACTOR = 16.0


def _restart_at(L):
    return 2 * L + 3


def _run(rec, series, restart=None, envs=None):
    """Feed ``series [n, B, S]`` (``envs``: views of those rows only); ``restart = (sample, envs)``."""
    gpu = isinstance(rec, SignalSpectra)
    dev = torch.as_tensor(series).cuda() if gpu else None
    for i in range(len(series)):
        if restart is not None and i == restart[0]:
            rec.restart(restart[1])
        smp = dev[i] if gpu else series[i]
        if envs is not None:
            smp = smp[envs]
        rec.update(smp[:, :WIDTHS[0]], smp[:, WIDTHS[0]:])                 # the sources are strided views of one row: read in place
    if gpu:
        torch.cuda.synchronize()
    return rec


def _errors(got, want):
    """Per signal and pair ``max |got - want| / max |want|`` over the envs' bins, for (power, cross, last)."""
    out = []
    for g, w in zip(got[:3], want[:3]):
        if w.ndim == 4:
            g, w = g[..., 0] + 1j * g[..., 1], w[..., 0] + 1j * w[..., 1]
        assert np.isfinite(g).all()
        scale = np.abs(w).max(axis=-1, keepdims=True)
        out.append(float((np.abs(g - w) / scale).max()) if g.size else 0.0)
    return out


class SinglePrecisionTwin(HostSignalSpectra):
    """The twin with its transform in single precision (``scipy.fft.rfft`` of a float32 array): the yardstick of the fp32 library."""

    def update(self, *sources):
        import scipy.fft

        import fluidgym_amd.simulation.signal_spectra as M

        def spectra(seg, window, detrend, dtype):
            v = np.asarray(seg, np.float64)
            n = v.shape[-1]
            tc = np.arange(n) - 0.5 * (n - 1)
            mean = v.sum(axis=-1, keepdims=True) / n if detrend else 0.0
            slope = (v * tc).sum(axis=-1, keepdims=True) / (n * (float(n) * n - 1.0) / 12.0) if detrend == 2 else 0.0
            y = ((v - (mean + slope * tc)) * window).astype(np.float32)
            X = scipy.fft.rfft(y, axis=-1)
            assert X.dtype == np.complex64
            return X.astype(np.complex128)

        keep, M.segment_spectra = M.segment_spectra, spectra
        try:
            super().update(*sources)
        finally:
            M.segment_spectra = keep


def _bound(lib, series, spec, restart, want):
    if lib == "fp64":
        return [BOUND_FP64] * 3
    ref = _run(SinglePrecisionTwin(*spec), series, restart)
    errs = _errors(ref._state(), want)
    print("   single-precision rfft against the twin: power %.2e cross %.2e last %.2e" % tuple(errs))
    return [FP32_FACTOR * e for e in errs]


CASES = [(L, ov, d) for L in (16, 32, 64) for ov in ("0", "L/2", "3L/4") for d in DETRENDS] + [(1024, "L/2", "linear")]


@pytest.mark.parametrize("lib", list(DTYPES))
@pytest.mark.parametrize("L,overlap,detrend", CASES)
def test_the_kernel_equals_the_twin_with_the_envs_out_of_phase(L, overlap, detrend, lib):
    noverlap = {"0": 0, "L/2": L // 2, "3L/4": 3 * L // 4}[overlap]
    series = batch_series(3, WIDTHS, L, seed=1, dtype=DTYPES[lib])
    spec = (NAMES, L, noverlap, "hann", detrend, PAIRS, 0.1)
    restart = (_restart_at(L), [1])
    twin = _run(HostSignalSpectra(*spec), series, restart)
    rec = _run(SignalSpectra(*spec), series, restart)
    got, want = rec._state(), twin._state()
    assert got[3].tolist() == want[3].tolist() and got[3].min() >= 2       # (env 1's segments fall on other samples, 3 later)
    errs, bounds = _errors(got, want), _bound(lib, series, spec, restart, want)
    print(f"{lib} L {L} noverlap {noverlap} {detrend}: power {errs[0]:.2e} cross {errs[1]:.2e} last {errs[2]:.2e}; bounds "
          f"{bounds[0]:.2e} {bounds[1]:.2e} {bounds[2]:.2e}")
    assert errs[0] <= bounds[0] and errs[1] <= bounds[1] and errs[2] <= bounds[2]
    # `last` is the power of the final segment: the sums of a fresh record fed that segment alone
    hop = L - noverlap
    for e in range(3):
        n = len(series) - (restart[0] if e == 1 else 0)
        end = len(series) - (n - L) % hop
        tail = _run(SignalSpectra(*spec), series[end - L:end, e:e + 1])
        assert tail._state()[0].tobytes() == got[2][e:e + 1].tobytes()
    # the cross spectrum of a signal with itself is its power, bit for bit
    assert got[1][:, 2, :, 0].tobytes() == got[0][:, 2].tobytes() and not got[1][:, 2, :, 1].any()
    assert np.array_equal(rec.psd("s3"), rec.record().psd("s3")) and rec.psd("s3").shape == (3, L // 2 + 1)


@pytest.mark.parametrize("lib", list(DTYPES))
@pytest.mark.parametrize("L,noverlap", [(16, 12), (32, 0), (64, 32)])
def test_an_env_does_not_depend_on_the_batch_around_it(L, noverlap, lib):
    series = batch_series(3, WIDTHS, L, seed=2, dtype=DTYPES[lib])
    spec = (NAMES, L, noverlap, "hann", "linear", PAIRS, 0.1)
    restart = (_restart_at(L), [1])
    whole = _run(SignalSpectra(*spec), series, restart)._state()
    for e in range(3):
        alone = _run(SignalSpectra(*spec), series, (restart[0], [0]) if e == 1 else None, envs=slice(e, e + 1))._state()
        for a, w in zip(alone, whole):
            assert a.tobytes() == w[e:e + 1].tobytes(), e
    twins = series.copy()
    twins[:, 2] = twins[:, 0]                                   # envs 0 and 2 identical, env 1 (restarted) between them
    got = _run(SignalSpectra(*spec), twins, restart)._state()
    for a, w in zip(got, whole):
        assert a[0].tobytes() == a[2].tobytes() == w[0].tobytes()


@pytest.mark.parametrize("lib", list(DTYPES))
@pytest.mark.parametrize("value", [np.nan, np.inf])
def test_a_non_finite_sample_marks_its_signal_and_its_pairs_and_nothing_else(value, lib):
    L, noverlap = 16, 8
    series = batch_series(3, WIDTHS, L, seed=3, dtype=DTYPES[lib])
    spec = (NAMES, L, noverlap, "hann", "constant", PAIRS + (("s2", "s3"),), 0.1)
    clean = _run(SignalSpectra(*spec), series)._state()
    bad = series.copy()
    bad[L + 5, 0, 2] = value
    got = _run(SignalSpectra(*spec), bad)._state()
    twin = _run(HostSignalSpectra(*spec), bad)._state()
    assert np.isnan(got[0][0, 2]).all() and np.isnan(got[1][0, 2]).all() and np.isnan(got[1][0, 3]).all()
    assert np.isfinite(got[2]).all()                            # the sample has left the ring: the last segment is whole again
    for g, t in zip(got[:3], twin[:3]):
        assert np.array_equal(np.isnan(g), np.isnan(t))
    keep_sig, keep_pair = [0, 1, 3, 4], [0, 1]
    assert got[0][0, keep_sig].tobytes() == clean[0][0, keep_sig].tobytes()
    assert got[1][0, keep_pair].tobytes() == clean[1][0, keep_pair].tobytes()
    for g, c in zip(got, clean):
        assert g[1:].tobytes() == c[1:].tobytes()
    assert got[2].tobytes() == clean[2].tobytes() and got[3].tolist() == clean[3].tolist()


def test_what_the_device_refuses_at_the_first_sample():
    with pytest.raises(ValueError, match="at most 2048"):
        SignalSpectra(("a",), 4096).update(torch.zeros(2, dtype=torch.float64, device="cuda"))
    rec = SignalSpectra(("a", "b"), 16)
    with pytest.raises(ValueError, match="the sources hold 3 signals"):
        rec.update(torch.zeros(2, 3, device="cuda"))
    rec.update(torch.zeros(2, device="cuda"), torch.ones(2, 1, device="cuda"))
    with pytest.raises(ValueError, match="changed between updates"):
        rec.update(torch.zeros(3, 2, device="cuda"))
    with pytest.raises(TypeError, match="one dtype and device"):
        rec.update(torch.zeros(2, device="cuda"), torch.ones(2, dtype=torch.float64, device="cuda"))
    rec.restart()
    rec.restart([1])
    assert rec.segments.tolist() == [0, 0] and np.isnan(rec.psd("a")).all()
    wide = SignalSpectra(("a",), 4096, 0, np.ones(4096), "none")          # the longest fp32 segment: one working wave
    x = torch.zeros(4096, 1, device="cuda")
    x[1] = 1.0
    for i in range(4096):
        wide.update(x[i])
    assert wide.segments.tolist() == [1] and np.abs(wide._state()[0] - 1.0).max() <= 1e-6      # a unit pulse: |X_k| = 1


# ---- the env layer
KW_CYL = dict(resolution=8, initial_domain_steps=6, randomize_initial_state=False, step_length=0.05, dt=0.01, episode_length=40)
KW_RBC = dict(n_heaters=4, resolution=8, step_length=0.1, load_initial_domain=False, load_domain_statistics=False,
              randomize_initial_state=False)


def _env_case(family):
    if family == "cylinder":
        env = fluidgym_amd.make("CylinderJet2D-easy-v0", num_envs=2, **KW_CYL)
        env.reset(seed=1)
        centres = env._require_multi_block("test").tables.centres
        point = np.asarray(centres[len(centres) // 3], np.float64)[None]
        located = env.locate_probes(point)
        return env, point, (lambda: located.sample(("u", "p")).flatten(1)), (lambda: env.reset_mesh_envs([1], randomize=False))
    env = fluidgym_amd.make("RBC2D-easy-v0", num_envs=2, **KW_RBC)
    env.reset(seed=3)
    from fluidgym_amd.simulation.tracers import PointGrid

    g = PointGrid(env._domain)
    point = (np.asarray(g.lo, np.float64) + 0.37 * np.asarray(g.len, np.float64))[None]
    return env, point, (lambda: env.probe(point, ("u", "p")).flatten(1)), (lambda: env.reset_envs([1]))


@pytest.mark.parametrize("family", ["cylinder", "rbc"])
def test_the_env_records_what_its_signals_returned(family):
    env, point, probe_now, restart_one = _env_case(family)
    log = []

    def wake(e):                                                # two columns of the state, logged with the probe of the same moment
        v = e._domain.velocity if family == "cylinder" else e._domain.getBlock(0).velocity
        out = torch.stack([v[:, 0].flatten(1)[:, 5], v[:, 1].flatten(1).mean(dim=1)], dim=1)
        log.append(torch.cat([out, probe_now()], dim=1).cpu().numpy())
        return out

    signals = [("wake", wake)] + (["lift"] if family == "cylinder" else [])
    pairs = [("wake[0]", "wake[1]"), ("wake[1]", "p@0")] + ([("lift", "u@0")] if family == "cylinder" else [])
    rec = env.start_signal_spectra(signals, probes=point, probe_fields=("u", "p"), segment=16, noverlap=8, pairs=pairs, every=1)
    assert env.signal_spectra is rec
    assert rec.names == ("wake[0]", "wake[1]") + (("lift",) if family == "cylinder" else ()) + ("u@0", "p@0")
    sim_dt = float(env._sim.time_step) if family == "cylinder" else env._sim_step_time()
    assert rec.dt == sim_dt
    del log[:]                                                  # (the evaluation that told start_* the width)
    lift_log = []
    if family == "cylinder":                                    # the built-in is logged through the env's own entry
        inner = env._get_drag_and_lift

        def logged():
            cd, cl = inner()
            lift_log.append(cl.cpu().numpy())
            return cd, cl
        env._get_drag_and_lift = logged
    action = torch.zeros(env._zero_action.shape, device=env.cuda_device)
    cut = None
    for step in range(40):
        if len(log) >= 44:
            break
        if cut is None and len(log) >= 19:                      # inside env 1's second segment
            restart_one()
            cut = len(log)
        env.step(action)
    assert cut is not None and len(log) >= 44
    if family == "cylinder":
        assert len(lift_log) == len(log)
        series = [np.concatenate([a[:, :2], l[:, None], a[:, 2:]], axis=1) for a, l in zip(log, lift_log)]
    else:
        series = log
    twin = HostSignalSpectra(rec.names, 16, 8, "hann", "constant", pairs, rec.dt)
    for i, smp in enumerate(series):
        if i == cut:
            twin.restart([1])
        twin.update(smp.astype(np.float32))
    torch.cuda.synchronize()
    got, want = rec._state(), twin._state()
    n0, n1 = 1 + (len(log) - 16) // 8, 1 + (cut - 16) // 8 + 1 + (len(log) - cut - 16) // 8
    assert got[3].tolist() == want[3].tolist() == [n0, n1] and n0 != n1 and min(n0, n1) >= 3
    spec = (rec.names, 16, 8, "hann", "constant", pairs, rec.dt)
    ref = SinglePrecisionTwin(*spec)
    for i, smp in enumerate(series):
        if i == cut:
            ref.restart([1])
        ref.update(smp.astype(np.float32))
    bounds = [FP32_FACTOR * e for e in _errors(ref._state(), want)]
    errs = _errors(got, want)
    print(f"{family}: power {errs[0]:.2e} cross {errs[1]:.2e} last {errs[2]:.2e}; bounds {bounds[0]:.2e} {bounds[1]:.2e} {bounds[2]:.2e}")
    assert errs[0] <= bounds[0] and errs[1] <= bounds[1] and errs[2] <= bounds[2]
    assert np.isfinite(rec.peak_frequency("wake[0]")).all() and rec.coherence("wake[1]", "p@0").shape == (2, 9)
    # stopped: a further step samples nothing
    stopped = env.stop_signal_spectra()
    assert stopped is rec and env.signal_spectra is None
    before, n_log = stopped._state(), len(log)
    fill = stopped._dev[5].clone()
    env.step(action)
    torch.cuda.synchronize()
    assert len(log) == n_log and torch.equal(stopped._dev[5], fill)
    assert stopped.segments.tolist() == before[3].tolist() and stopped._state()[0].tobytes() == before[0].tobytes()
    with pytest.raises(RuntimeError, match="no signal spectra are being recorded"):
        env.stop_signal_spectra()
    env.close()
