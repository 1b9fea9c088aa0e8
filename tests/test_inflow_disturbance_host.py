"""Per-env unsteady inflow without a GPU: the NumPy restatement of ``fg_mb_inflow_disturbance``
(``tests/inflow_disturbance_ref.py``) against an extended-precision evaluation, the drawn modes, the refusals of ``InflowDisturbance`` and
of the entry point (status codes from host-only handles, before any launch), the ``state_dict`` round trip, the counters an env hands
the kernel, and the refusing stubs."""
import ctypes
import math
from types import SimpleNamespace

import numpy as np
import pytest

from fluidgym_amd import _lib as L
from fluidgym_amd.envs.inflow import InflowDisturbanceMixin
from fluidgym_amd.simulation.inflow_disturbance import MAX_MODES, InflowDisturbance
from tests import inflow_disturbance_ref as R

LD = np.longdouble
SWEEP_N = [0, 1, 2, 3, 17, 999, 10 ** 5, 10 ** 7, 10 ** 7 + 1]
SWEEP_DT = [0.01, 0.004, 0.0125]
MEASURED_SINE_ERROR = 2.2048e-07      # worst |restatement - extended-precision sine| over the sweep below, measured on the CPU


def _exact_sine(f, n, dt, phi):
    """sin 2 pi (f n dt + phi) with the phase formed in extended precision from the integer step count: no cycle is lost."""
    x = LD(f) * LD(n) * LD(dt) + LD(phi)
    return np.sin(2 * np.arccos(LD(-1)) * (x - np.floor(x)))


def test_restatement_against_the_fp64_evaluation():
    """The fp32 sine of the double phase over (n, dt, f, phi), n up to 10^7 + 1 (300 000 cycles at f = 3: a phase held in fp32 would
    have lost them).  Measured worst error on the CPU against the extended-precision sine: 2.2048e-07 (the polynomials' own error plus
    the rounding of the phase to fp32); the bound is twice that and covers only the sampling of the sweep, since the kernel is held
    to the restatement's bits."""
    f = np.linspace(0.0, 3.0, 257)[:, None]
    phi = np.linspace(0.0, 1.0, 64, endpoint=False)[None, :]
    worst = 0.0
    for n in SWEEP_N:
        for dt in SWEEP_DT:
            r = R.sin2pi_frac(f * R.time_of(n, dt) + phi)
            worst = max(worst, float(np.abs(r.astype(LD) - _exact_sine(f, n, dt, phi)).max()))
    print(f"worst sine error over the sweep: {worst:.4e}")
    assert worst <= 2.0 * MEASURED_SINE_ERROR
    # the signals are sums of at most 8 such terms with sum |a_k| <= 0.9: the same bound times 0.9, plus the fp32 sum's rounding
    modes = R.draw_modes(11, 2, 3, 8, 8, (0.05, 2.0), 0.1, 0.05)
    y = np.linspace(-2.0, 2.0, 33)
    for n in SWEEP_N:
        t = R.time_of(n, 0.0125)
        a, fr, ph, g, h, psi = modes
        S = R.streamwise(a, fr, ph, t)
        S64 = float(np.sum(a.astype(LD) * _exact_sine(fr, n, 0.0125, ph)))
        assert abs(float(S) - S64) <= 0.9 * 2.0 * MEASURED_SINE_ERROR + 8 * 2.0 ** -24
        assert abs(float(S) - R.streamwise_f64(a, fr, ph, t)) <= 0.9 * 2.0 * MEASURED_SINE_ERROR + 8 * 2.0 ** -24
        G = R.transverse(g, h, psi, 0.3, t, y)
        assert np.abs(G.astype(np.float64) - R.transverse_f64(g, h, psi, 0.3, t, y)).max() <= 0.9 * 2.0 * MEASURED_SINE_ERROR + 8 * 2.0 ** -24


def test_sine_edges():
    """Whole and half cycles are exact zeros, quarter cycles exact ones, and a phase that rounds to 1.0f folds to zero."""
    x = np.array([0.0, 0.25, 0.5, 0.75, 1.0, 7.25, -0.25, -1e-30, 123456.5])
    assert R.sin2pi_frac(x).tolist() == [0.0, 1.0, 0.0, -1.0, 0.0, 1.0, -1.0, 0.0, 0.0]


def test_random_draws():
    band, ks, kt = (0.05, 0.45), 5, 3
    for seed, row, ep in [(0, 0, 0), (2 ** 40 + 5, 17, 3), (9, 2 ** 31 - 1, 2 ** 32 - 1)]:
        a, f, phi, g, h, psi = R.draw_modes(seed, row, ep, ks, kt, band, 0.1, 0.02)
        for k in range(ks):
            assert band[0] + k * 0.4 / ks <= f[k] <= band[0] + (k + 1) * 0.4 / ks
        for k in range(kt):
            assert band[0] + k * 0.4 / kt <= h[k] <= band[0] + (k + 1) * 0.4 / kt
        assert ((phi > 0) & (phi < 1)).all() and ((psi > 0) & (psi < 1)).all()
        assert a.dtype == np.float32 and np.all(a == np.float32(0.1 * np.sqrt(2.0 / ks))) and np.all(g == np.float32(0.02 * np.sqrt(2.0 / kt)))
        # the rms of the streamwise signal is streamwise_rms: sum a_k^2 / 2
        assert math.isclose(float(np.sum(a.astype(np.float64) ** 2) / 2), 0.1 ** 2, rel_tol=1e-6)
    # a pure function of (seed, row, episode): nothing else enters, so no batch size does; the others each change the draw
    ref = R.draw_modes(5, 3, 2, 4, 4, band, 0.1, 0.1)
    same = R.draw_modes(5, 3, 2, 4, 4, band, 0.1, 0.1)
    assert all(np.array_equal(x, y) for x, y in zip(ref, same))
    for other in [(6, 3, 2), (5, 4, 2), (5, 3, 3)]:
        assert not np.array_equal(R.draw_modes(*other, 4, 4, band, 0.1, 0.1)[1], ref[1])
    # env_offset shifts the rows: row r of offset 0 is row r - 2 of offset 2 (the kernel adds the offset to the env index)
    big = R.batch_modes(5, 0, [0, 1, 2, 3, 4], 5, 4, 4, band, 0.1, 0.1)
    small = R.batch_modes(3, 2, [2, 3, 4], 5, 4, 4, band, 0.1, 0.1)
    assert all(np.array_equal(x, y) for b in range(3) for x, y in zip(big[2 + b], small[b]))
    # streamwise mode k and transverse mode k share a Philox block but not its words
    assert not np.array_equal(ref[2], ref[5])


def test_spec_refusals_and_forms():
    with pytest.raises(ValueError, match="reverse"):
        InflowDisturbance(a=[0.5, -0.41], f=[0.1, 0.2], phi=[0.0, 0.0])
    InflowDisturbance(a=[0.5, -0.4], f=[0.1, 0.2], phi=[0.0, 0.0])
    with pytest.raises(ValueError, match="reverse"):
        InflowDisturbance(a=[[0.1], [0.95]], f=[0.1], phi=[0.0])                 # one env of a per-env table
    with pytest.raises(ValueError, match="reverse"):
        InflowDisturbance.random(0, n_streamwise=8, streamwise_rms=0.23)          # 8 * 0.23 sqrt(2 / 8) = 0.92
    with pytest.raises(ValueError, match="at most 8"):
        InflowDisturbance(a=[0.01] * 9, f=[0.1] * 9, phi=[0.0] * 9)
    with pytest.raises(ValueError, match="outside 0..8"):
        InflowDisturbance.random(0, n_streamwise=9)
    with pytest.raises(ValueError, match="outside 0..8"):
        InflowDisturbance.random(0, n_transverse=9)
    with pytest.raises(ValueError, match="non-negative"):
        InflowDisturbance(a=[0.1], f=[-0.1], phi=[0.0])
    with pytest.raises(ValueError, match="non-negative"):
        InflowDisturbance(g=[0.1], h=[-0.1], psi=[0.0])
    with pytest.raises(ValueError, match="non-negative"):
        InflowDisturbance.random(0, band=(-0.1, 0.5))
    with pytest.raises(ValueError, match="finite"):
        InflowDisturbance(a=[0.1], f=[math.inf], phi=[0.0])
    with pytest.raises(ValueError, match="finite"):
        InflowDisturbance.random(0, band=(0.1, math.nan))
    with pytest.raises(ValueError, match="same number"):
        InflowDisturbance(a=[0.1, 0.1], f=[0.1], phi=[0.0])
    spec = InflowDisturbance(a=[[0.1, 0.2], [0.3, 0.1], [0.0, 0.0]], f=[0.5, 1.0], phi=[0.0, 0.25], g=[0.05], h=[0.2], psi=[0.5], kappa=0.3)
    t = spec.modes_table(3)
    assert t.shape == (3, 6, MAX_MODES) and t.dtype == np.float64
    assert t[1, 0, :3].tolist() == [0.3, 0.1, 0.0] and t[2, 1, :2].tolist() == [0.5, 1.0] and t[0, 3, 0] == 0.05 and t[0, 5, 0] == 0.5
    with pytest.raises(ValueError, match="batch"):
        spec.modes_table(4)
    assert InflowDisturbance.random(1).modes_table(4) is None


def test_state_dict_round_trip():
    for spec in (InflowDisturbance(a=[[0.1, 0.2], [0.3, 0.1]], f=[0.5, 1.0], phi=[0.0, 0.25], g=[0.05], h=[0.2], psi=[0.5], kappa=0.3),
                 InflowDisturbance.random(2 ** 50 + 1, 3, 2, (0.1, 0.9), 0.07, 0.03, kappa=-0.5, env_offset=16)):
        d = spec.state_dict()
        for twin in (InflowDisturbance.from_state_dict(d), InflowDisturbance.random(0).load_state_dict(d)):
            d2 = twin.state_dict()
            assert d2.keys() == d.keys() and twin.form == spec.form
            for k in d:
                if k == "tables":
                    assert all(np.array_equal(d[k][x], d2[k][x]) for x in d[k])
                else:
                    assert d[k] == d2[k], k
            assert (twin.n_streamwise, twin.n_transverse, twin.kappa) == (spec.n_streamwise, spec.n_transverse, spec.kappa)


def test_counters_come_from_the_envs_own_counters():
    """n_b = episode_steps[b] * n_sim_steps + k and e_b = mesh_reset_count[b]: the words the env uploads once per env step."""
    env = SimpleNamespace(episode_steps=np.array([0, 5, 2 ** 32 + 3], np.int64), mesh_reset_count=np.array([0, 2, 7], np.int64))
    w = InflowDisturbanceMixin._inflow_counter_words(env)
    assert w.dtype == np.uint32 and w.tolist() == [[0, 0], [5, 2], [3, 7]]
    # the time the kernel forms from them: (steps * sim_steps + k) dt
    assert float(R.time_of(int(w[1, 0]) * 4 + 3, 0.0125)) == 23 * 0.0125


def _coords(nx, ny, dtype):
    x, y = np.linspace(0, 1, nx + 1), np.linspace(0, 1, ny + 1)
    return np.ascontiguousarray(np.stack(np.meshgrid(x, y, indexing="xy")).astype(dtype))


LIBS = [("f32", L.load, ctypes.c_float), ("f64", L.load_f64, ctypes.c_double)]


@pytest.mark.parametrize("name,load,real", LIBS, ids=[n for n, _, _ in LIBS])
def test_entry_refuses_by_code_without_a_gpu(name, load, real):
    """Every refusal is a status code with a message, before any launch: the pointers are never dereferenced.  One block of 3 x 4
    cells with every face FIXED: slots -x 0..3, +x 4..7, -y 8..10, +y 11..13."""
    lib = load()
    assert hasattr(lib, "fg_mb_inflow_disturbance")
    assert "fg_mb_inflow_disturbance" in L.SIGNATURES and "fg_mb_inflow_disturbance" in L.SIGNATURES_F64
    assert ctypes.sizeof(L.FgMbInflowParams) == 12 * 4 + 8 + 8 * 8 + 5 * 8
    h, raw = ctypes.c_void_p(), ctypes.c_void_p()
    for handle in (h, raw):
        assert lib.fg_mb_create(2, 3, -1, ctypes.byref(handle)) == 0
        c = _coords(3, 4, np.float64 if real is ctypes.c_double else np.float32)
        assert lib.fg_mb_add_block(handle, c.ctypes.data_as(ctypes.POINTER(real)), 3, 4, 1, None) == 0
    assert lib.fg_mb_finalize(h) == 0

    def call(handle=h, null=False, **kw):
        p = L.FgMbInflowParams(slot0=0, count=4, outflow_slot0=4, outflow_count=4, n_streamwise=2, n_transverse=1, sim_steps=4, k=1,
                               seed=7, dt=0.01, f_lo=0.1, f_hi=0.5, streamwise_rms=0.1, transverse_rms=0.05, outflow_tol=5e-6,
                               base=0x1000, y=0x2000, counters=0x3000, signal=0x4000)
        for key, v in kw.items():
            setattr(p, key, v)
        rc = lib.fg_mb_inflow_disturbance(handle, None if null else ctypes.byref(p), None)
        return rc, lib.fg_last_error().decode()

    try:
        bad = L.FG_ERR_INVALID_ARG
        for what, kw, word in [
            ("null handle", dict(handle=None), "null handle"),
            ("null parameters", dict(null=True), "null parameters"),
            ("K_s > 8", dict(n_streamwise=9), "0..8"),
            ("K_t > 8", dict(n_transverse=9), "0..8"),
            ("K < 0", dict(n_streamwise=-1), "0..8"),
            ("count = 0", dict(count=0), "count"),
            ("count < 0", dict(count=-2), "count"),
            ("dt nan", dict(dt=math.nan), "dt"),
            ("dt inf", dict(dt=math.inf), "dt"),
            ("dt < 0", dict(dt=-0.01), "dt"),
            ("k past the env step", dict(k=4), "sim_steps"),
            ("sim_steps = 0", dict(sim_steps=0, k=0), "sim_steps"),
            ("kappa nan", dict(kappa=math.nan), "finite"),
            ("band reversed", dict(f_lo=0.5, f_hi=0.1), "band"),
            ("band negative", dict(f_lo=-0.1), "band"),
            ("rms negative", dict(streamwise_rms=-0.1), "band"),
            ("null base", dict(base=None), "null base"),
            ("null y", dict(y=None), "null base"),
            ("null counters", dict(counters=None), "null base"),
            ("null signal", dict(signal=None), "null base"),
            ("inflow past NB", dict(slot0=12, count=4), "inflow slots"),
            ("inflow slot0 < 0", dict(slot0=-1), "inflow slots"),
            ("outflow past NB", dict(outflow_slot0=11, outflow_count=4), "outflow slots"),
            ("no outflow", dict(outflow_count=0), "outflow slots"),
            ("second outflow past NB", dict(outflow_slot0_b=13, outflow_count_b=2), "outflow slots"),
            ("inflow overlaps outflow", dict(slot0=2, count=4), "overlap"),
            ("outflows overlap", dict(outflow_slot0_b=6, outflow_count_b=3), "overlap"),
        ]:
            rc, msg = call(**kw)
            assert rc == bad and "fg_mb_inflow_disturbance" in msg and word in msg, (what, rc, msg)
        # valid calls end at the bound-field check: both forms, zero amplitude, two outflow ranges; an unfinalised handle likewise
        unbound = L.FG_ERR_NOT_BOUND
        assert call()[0] == unbound and call(modes=0x5000)[0] == unbound
        assert call(n_streamwise=0, n_transverse=0)[0] == unbound and call(n_streamwise=8, n_transverse=8)[0] == unbound
        assert call(outflow_slot0_b=11, outflow_count_b=3)[0] == unbound
        assert call(modes=0x5000, f_lo=math.nan)[0] == unbound                      # the band belongs to the random form
        assert call(handle=raw)[0] == unbound
    finally:
        assert lib.fg_mb_destroy(h) == 0 and lib.fg_mb_destroy(raw) == 0


def test_refusing_stubs():
    from fluidgym_amd.envs.fluid_env import FluidEnv
    from fluidgym_amd.envs.parallel_env import ParallelFluidEnv

    fake = SimpleNamespace(_refuse_inflow_disturbance=lambda entry: FluidEnv._refuse_inflow_disturbance(fake, entry))
    for entry in ("start_inflow_disturbance", "stop_inflow_disturbance", "inflow_signal"):
        with pytest.raises(NotImplementedError, match="cylinder, airfoil"):
            getattr(FluidEnv, entry)(fake)
        with pytest.raises(NotImplementedError, match="ParallelFluidEnv"):
            getattr(ParallelFluidEnv, entry)(None)
    assert FluidEnv.inflow_disturbance.fget(fake) is None
    # an env with the mixin and no disturbance: stop refuses like the other stop_* entries, the loop's call is a no-op
    idle = SimpleNamespace(_inflow_spec=None)
    with pytest.raises(RuntimeError, match="no inflow disturbance is active"):
        InflowDisturbanceMixin.stop_inflow_disturbance(idle)
    assert InflowDisturbanceMixin._before_sim_step(idle, 0) is None
