"""``fg_plane_histogram`` on the GPU, both libraries, against the NumPy checker (``tests/plane_hist_ref.py``): every comparison is
exact equality of ``uint64`` counters.  Then ``start_flow_histograms`` / ``stop_flow_histograms`` of the smallest RBC2D and TCF envs."""
import ctypes

import numpy as np
import pytest
import torch

import fluidgym_amd
from fluidgym_amd import _lib as L
from fluidgym_amd.simulation.plane_hist import PlaneHistograms
from tests import plane_hist_ref as ref

pytestmark = pytest.mark.gpu

B = 3
GUARD = 64                       # counters past the logical end of each accumulator
DTYPES = ((np.float32, torch.float32), (np.float64, torch.float64))
# (nz, ny, nx): 2-D planes of fewer cells than lanes and with a tail (15 rows: a workgroup with an idle wave), exactly 1024 cells
# (the last size one wave takes), 1060 cells with 16-byte loads, 1065 cells with scalar loads
SHAPES = {"2d-8": (1, 5, 8), "2d-65": (1, 5, 65), "3d-1024": (4, 3, 256), "3d-1060": (5, 3, 212), "3d-1065": (5, 3, 213)}
# K, bins, pairs, joint_bins (workgroup form, small-plane form)
PARAMS = {
    "K1-bins2": (1, 2, [], (2, 2)),
    "K5-bins256-3pairs": (5, 256, [(0, 1), (3, 3), (4, 1)], (64, 32)),          # the largest tables each form must support
    "K5-bins8-1pair": (5, 8, [(1, 2)], (2, 2)),
    "K2-bins12-ratio3": (2, 12, [(1, 0)], (4, 4)),                              # bins / joint_bins not a power of two
}


def _lib(np_dtype):
    return L.load_f64() if np_dtype == np.float64 else L.load()


def _tables(rows, K, bins, np_dtype):
    """Ranges that differ per listed row and channel, about [-1, 1]."""
    r, k = np.meshgrid(np.arange(len(rows)), np.arange(K), indexing="ij")
    lo, hi = -1.0 - 0.1 * r - 0.05 * k, 1.0 + 0.07 * r + 0.03 * k
    return lo, hi, ref.tables(lo, hi, bins, np_dtype)


def _normal(seed, K, shape, np_dtype):
    """Seeded normal data spread over about 1.5 times the range: the below and above slots fill."""
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal((B,) + shape) * 0.75).astype(np_dtype) for _ in range(K)]


class Launch:
    """The device side of one accumulator: fields placed in buffers (``offset`` reals before channel 0, ``pad`` reals between the
    envs), counters pre-filled with a pattern and followed by GUARD more."""

    def __init__(self, fields, rows, lo_real, scale, bins, pairs, jb, offset=0, pad=0):
        self.np_dtype = fields[0].dtype.type
        self.lib = _lib(self.np_dtype)
        self.K, (_, self.nz, self.ny, self.nx) = len(fields), fields[0].shape
        self.rows, self.bins, self.pairs, self.jb = list(rows), bins, list(pairs), jb
        field = self.nz * self.ny * self.nx
        self.stride = field + pad
        self.bufs, ptrs = [], []
        for k, f in enumerate(fields):
            off = offset if k == 0 else 0
            buf = torch.full((off + B * self.stride,), 7.0, dtype=torch.from_numpy(f).dtype, device="cuda")
            buf[off:].view(B, self.stride)[:, :field] = torch.from_numpy(f.reshape(B, field)).cuda()
            self.bufs.append(buf)
            ptrs.append(buf.data_ptr() + off * buf.element_size())
        self.ptrs = (ctypes.c_void_p * self.K)(*ptrs)
        self.strides = (ctypes.c_int64 * self.K)(*([self.stride] * self.K))
        self.lo, self.scale = torch.from_numpy(lo_real).cuda(), torch.from_numpy(scale).cuda()
        R, P = len(self.rows), len(self.pairs)
        self.n_counts, self.n_joint = B * R * self.K * (bins + 3), B * R * P * (jb * jb + 1)
        self.pat_c = np.arange(self.n_counts + GUARD, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) >> np.uint64(3)
        self.pat_j = np.arange(self.n_joint + GUARD, dtype=np.uint64) * np.uint64(0xC2B2AE3D27D4EB4F) >> np.uint64(3)
        self.counts = torch.from_numpy(self.pat_c.view(np.int64).copy()).cuda()
        self.joint = torch.from_numpy(self.pat_j.view(np.int64).copy()).cuda()

    def __call__(self):
        R, P = len(self.rows), len(self.pairs)
        rows = (ctypes.c_int32 * R)(*self.rows)
        pairs = (ctypes.c_int32 * max(2 * P, 1))(*[i for p in self.pairs for i in p])
        rc = self.lib.fg_plane_histogram(self.ptrs, self.strides, self.K, B, self.nz, self.ny, self.nx, rows, R,
                                         ctypes.c_void_p(self.lo.data_ptr()), ctypes.c_void_p(self.scale.data_ptr()), self.bins, pairs, P,
                                         self.jb, ctypes.c_void_p(self.counts.data_ptr()),
                                         ctypes.c_void_p(self.joint.data_ptr()) if P else None, None)
        L.check(rc, lib=self.lib)

    def read(self):
        """The counters added since the pattern was written (the guards must be untouched)."""
        torch.cuda.synchronize()
        c, j = self.counts.cpu().numpy().view(np.uint64), self.joint.cpu().numpy().view(np.uint64)
        assert np.array_equal(c[self.n_counts:], self.pat_c[self.n_counts:]), "counts: written past the end"
        assert np.array_equal(j[self.n_joint:], self.pat_j[self.n_joint:]), "joint: written past the end"
        R, P = len(self.rows), len(self.pairs)
        return ((c - self.pat_c)[:self.n_counts].reshape(B, R, self.K, self.bins + 3),
                (j - self.pat_j)[:self.n_joint].reshape(B, R, P, self.jb * self.jb + 1))


def _check(fields, rows, bins, pairs, jb, samples=1, **place):
    """``samples`` launches on the same fields against ``samples`` times the checker; returns the checker's one-sample tables."""
    np_dtype = fields[0].dtype.type
    _, _, (lo_real, scale) = _tables(rows, len(fields), bins, np_dtype)
    run = Launch(fields, rows, lo_real, scale, bins, pairs, jb, **place)
    for _ in range(samples):
        run()
    got_c, got_j = run.read()
    want_c, want_j = ref.histogram(fields, rows, lo_real, scale, bins, pairs, jb)
    assert np.array_equal(got_c, want_c * np.uint64(samples))
    assert np.array_equal(got_j, want_j * np.uint64(samples))
    cells = fields[0].shape[1] * fields[0].shape[3]
    assert (got_c.sum(axis=-1) == samples * cells).all() and (got_j.sum(axis=-1) == samples * cells).all()
    return want_c, want_j


def _row_choices(ny):
    return (list(range(ny)), [0, ny - 1], [ny // 2])


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("params", PARAMS)
def test_normal_data_every_shape_parameter_and_row_choice(shape, params):
    nz, ny, nx = SHAPES[shape]
    K, bins, pairs, jbs = PARAMS[params]
    jb = jbs[1] if nz * nx <= 1024 else jbs[0]
    for np_dtype, _ in DTYPES:
        fields = _normal(nx + K, K, (nz, ny, nx), np_dtype)
        for rows in _row_choices(ny):
            want_c, _ = _check(fields, rows, bins, pairs, jb)
            if len(rows) == ny:
                assert want_c[..., 0].any() and want_c[..., bins + 1].any() and want_c[..., 1:bins + 1].any()


@pytest.mark.parametrize("shape", ("2d-65", "3d-1024", "3d-1060", "3d-1065"))
def test_every_cell_in_one_bin(shape):
    """The most contended case: every lane of every wave adds to the same LDS counter."""
    nz, ny, nx = SHAPES[shape]
    for np_dtype, _ in DTYPES:
        fields = [np.full((B, nz, ny, nx), 0.25 + 0.125 * k, np_dtype) for k in range(3)]
        want_c, want_j = _check(fields, list(range(ny)), 8, [(0, 1), (2, 2)], 4)
        assert (want_c.max(axis=-1) == nz * nx).all() and (want_j.max(axis=-1) == nz * nx).all()


@pytest.mark.parametrize("shape", ("2d-65", "3d-1060"))
def test_cells_at_the_edges_and_one_ulp_either_side(shape):
    nz, ny, nx = SHAPES[shape]
    for np_dtype, _ in DTYPES:
        rows = list(range(ny))
        lo, hi, (lo_real, _) = _tables(rows, 2, 8, np_dtype)
        inf = np_dtype(np.inf)
        edge = np.empty((2, B, nz, ny, nx), np_dtype)
        for k in range(2):
            for r in rows:
                l, h = lo_real[r, k], np_dtype(hi[r, k])
                vals = np.array([l, np.nextafter(l, -inf), np.nextafter(l, inf), h, np.nextafter(h, -inf), np.nextafter(h, inf),
                                 np_dtype(0.0), np_dtype(0.5) * (l + h)], np_dtype)
                edge[k, :, :, r, :] = np.resize(np.roll(vals, k), (B, nz, nx))
        want_c, _ = _check([edge[0], edge[1]], rows, 8, [(0, 1)], 2)
        assert want_c[..., 0].any() and want_c[..., 1].any() and want_c[..., 9].any()


@pytest.mark.parametrize("shape", ("2d-8", "3d-1024", "3d-1065"))
def test_non_finite_cells_stay_in_their_row(shape):
    nz, ny, nx = SHAPES[shape]
    for np_dtype, _ in DTYPES:
        clean = _normal(3, 3, (nz, ny, nx), np_dtype)
        dirty = [f.copy() for f in clean]
        bad = ny // 2
        dirty[0][1, 0, bad, 0] = np.nan
        dirty[1][1, nz - 1, bad, nx - 1] = np.inf
        dirty[1][1, 0, bad, 1] = -np.inf
        dirty[2][1, :, bad, :] = np.nan
        rows, pairs = list(range(ny)), [(0, 1), (1, 2)]
        want_clean = _check(clean, rows, 16, pairs, 4)
        want_dirty = _check(dirty, rows, 16, pairs, 4)
        assert want_dirty[0][1, bad, 0, 18] == 1 and want_dirty[0][1, bad, 2, 18] == nz * nx and want_dirty[1][1, bad, 1, -1] == nz * nx
        assert want_dirty[0][1, bad, 1, 0] >= 1 and want_dirty[0][1, bad, 1, 17] >= 1
        keep = np.ones((B, ny), bool)
        keep[1, bad] = False
        for a, b in zip(want_clean, want_dirty):         # (the device equals the checker in both runs: the other rows are unaffected)
            assert np.array_equal(a[keep], b[keep])


@pytest.mark.parametrize("shape", ("2d-65", "3d-1060"))
def test_three_launches_accumulate(shape):
    nz, ny, nx = SHAPES[shape]
    for np_dtype, _ in DTYPES:
        rows, bins, pairs, jb = [0, ny - 1], 32, [(0, 2)], 8
        _, _, (lo_real, scale) = _tables(rows, 3, bins, np_dtype)
        samples = [_normal(20 + s, 3, (nz, ny, nx), np_dtype) for s in range(3)]
        run = Launch(samples[0], rows, lo_real, scale, bins, pairs, jb)
        want_c = want_j = 0
        for s, fields in enumerate(samples):
            for buf, f in zip(run.bufs, fields):
                buf.view(B, -1)[:] = torch.from_numpy(f.reshape(B, -1)).cuda()
            run()
            c, j = ref.histogram(fields, rows, lo_real, scale, bins, pairs, jb)
            want_c, want_j = want_c + c, want_j + j
        got_c, got_j = run.read()
        assert np.array_equal(got_c, want_c) and np.array_equal(got_j, want_j)
        assert (got_c.sum(axis=-1) == 3 * nz * nx).all()
        _check(samples[0], rows, bins, pairs, jb, samples=3)


@pytest.mark.parametrize("shape", ("2d-8", "3d-1024", "3d-1060"))
@pytest.mark.parametrize("place", (dict(offset=1), dict(pad=4), dict(pad=1), dict(offset=1, pad=3)))
def test_offset_channel_pointer_and_larger_batch_stride(shape, place):
    nz, ny, nx = SHAPES[shape]
    for np_dtype, _ in DTYPES:
        _check(_normal(9, 2, (nz, ny, nx), np_dtype), [0, ny - 1], 16, [(0, 1)], 8, **place)


def test_joint_marginals_are_the_coarsened_counts_on_the_device():
    nz, ny, nx = SHAPES["3d-1060"]
    for np_dtype, _ in DTYPES:
        rows, bins, jb = list(range(ny)), 24, 8
        fields = _normal(5, 2, (nz, ny, nx), np_dtype)
        fields[1][0, 0, 0, :7] = np.nan
        _, _, (lo_real, scale) = _tables(rows, 2, bins, np_dtype)
        run = Launch(fields, rows, lo_real, scale, bins, [(0, 1)], jb)
        run()
        _, got_j = run.read()
        for b in range(B):
            for r in rows:
                s = [ref.slots(np.ascontiguousarray(fields[k][b, :, r, :]), lo_real[r, k], scale[r, k], bins).ravel() for k in range(2)]
                both = (s[0] >= 1) & (s[0] <= bins) & (s[1] >= 1) & (s[1] <= bins)
                t = got_j[b, r, 0, :-1].reshape(jb, jb)
                assert np.array_equal(t.sum(axis=1), np.bincount((s[0][both] - 1) // 3, minlength=jb).astype(np.uint64))
                assert np.array_equal(t.sum(axis=0), np.bincount((s[1][both] - 1) // 3, minlength=jb).astype(np.uint64))
                assert got_j[b, r, 0, -1] == (~both).sum() and t.sum() + got_j[b, r, 0, -1] == nz * nx


@pytest.mark.parametrize("dims", (2, 3))
def test_recorder_class_reads_the_block_tensors_in_place(dims):
    """``PlaneHistograms.update`` on ``[B, d, (Z,) Y, X]`` tensors: component slices, pressure and scalar, per-row ranges."""
    rng = np.random.default_rng(dims)
    grid = (4, 5, 24) if dims == 3 else (5, 24)
    channels = ("u", "v", "w", "p", "T") if dims == 3 else ("u", "v", "p", "T")
    for np_dtype, t_dtype in DTYPES:
        vel = (rng.standard_normal((B, dims) + grid) * 0.75).astype(np_dtype)
        p = (rng.standard_normal((B, 1) + grid) * 0.75).astype(np_dtype)
        T = rng.uniform(-0.2, 1.2, (B, 2) + grid).astype(np_dtype)
        rows = [1, 3]
        ranges = {c: (-1.0, 1.0) for c in channels}
        ranges["u"] = np.array([[-1.0, 1.0], [-0.5, 1.5]])
        ranges["T"] = (0.0, 1.0)
        joint = (("u", "v"), ("v", "T"))
        acc = PlaneHistograms(channels, ranges, bins=32, joint=joint, joint_bins=8, rows=rows)
        for _ in range(2):
            acc.update(torch.from_numpy(vel).cuda(), torch.from_numpy(p).cuda(), torch.from_numpy(T).cuda())
        f = {"u": vel[:, 0], "v": vel[:, 1], "w": vel[:, dims - 1], "p": p[:, 0], "T": T[:, 0]}
        fields = [np.ascontiguousarray(f[c] if dims == 3 else f[c][:, None]) for c in channels]
        lo = np.stack([np.broadcast_to(ranges[c], (2, 2))[:, 0] for c in channels], axis=1)
        hi = np.stack([np.broadcast_to(ranges[c], (2, 2))[:, 1] for c in channels], axis=1)
        lo_real, scale = ref.tables(lo, hi, 32, np_dtype)
        want_c, want_j = ref.histogram(fields, rows, lo_real, scale, 32, [(channels.index(a), channels.index(b)) for a, b in joint], 8)
        assert acc.n_samples == 2
        for k, ch in enumerate(channels):
            assert np.array_equal(acc.counts(ch), 2 * want_c[:, :, k, 1:33]) and np.array_equal(acc.below(ch), 2 * want_c[:, :, k, 0])
            assert np.array_equal(acc.above(ch), 2 * want_c[:, :, k, 33]) and np.array_equal(acc.nonfinite(ch), 2 * want_c[:, :, k, 34])
        for q, (a, b) in enumerate(joint):
            assert np.array_equal(acc.joint_counts(a, b), 2 * want_j[:, :, q, :-1].reshape(B, 2, 8, 8))
            assert np.array_equal(acc.joint_outside(a, b), 2 * want_j[:, :, q, -1])
        host = acc.record()
        assert np.array_equal(host.merge(acc).counts("u"), 2 * acc.counts("u")) and host.n_samples == 4
        assert np.array_equal(acc.merge(acc.record()).counts("v"), 4 * want_c[:, :, 1, 1:33]) and acc.n_samples == 4
        with pytest.raises(ValueError, match="changed"):
            acc.update(torch.from_numpy(vel[:2]).cuda(), torch.from_numpy(p[:2]).cuda(), torch.from_numpy(T[:2]).cuda())


# ---- env level: the smallest envs the suite builds (tests/test_gpu_flow_statistics.py)

TCF = dict(num_envs=2, randomize_initial_state=False, resolution_x_z=16, resolution_y=16, step_length=0.6, use_marl=False)
RBC = dict(num_envs=2, n_heaters=4, resolution=8, randomize_initial_state=False, step_length=0.5)
ENVS = {"tcf": ("TCFSmall3D-both-easy-v0", TCF, 4, ("u", "v", "w", "p"), (("u", "v"),)),
        "rbc": ("RBC2D-easy-v0", RBC, 1, ("u", "v", "p", "T"), (("v", "T"),))}


def _flat(out):
    """The tensors and numbers of a step's outputs, in a fixed order."""
    if isinstance(out, dict):
        return [x for k in sorted(out) for x in _flat(out[k])]
    if isinstance(out, (tuple, list)):
        return [x for o in out for x in _flat(o)]
    return [out]


def _same(a, b):
    fa, fb = _flat(a), _flat(b)
    assert len(fa) == len(fb)
    for x, y in zip(fa, fb):
        if isinstance(x, torch.Tensor):
            assert torch.equal(x, y)
        elif isinstance(x, np.ndarray):
            assert np.array_equal(x, y)
        else:
            assert x == y or (x != x and y != y)


def _env_run(family, record):
    name, kw, seed, channels, joint = ENVS[family]
    env = fluidgym_amd.make(name, **kw)
    env.reset(seed=seed)
    action = torch.zeros(env._zero_action.shape if family == "tcf" else (2, 4, 1), device=env.cuda_device)
    hist = stats = fed = None
    if record:
        env.start_flow_histograms(bins=64, joint=joint, joint_bins=16)
        env.start_flow_statistics(order=2)
    outs = [env.step(action) for _ in range(2)]
    if record:
        hist, stats = env.stop_flow_histograms(), env.stop_flow_statistics()
        blk = env._block
        scalar = blk.passiveScalar if "T" in channels else None
        ranges = {c: np.stack([hist.lo[:, k], hist.hi[:, k]], axis=1) for k, c in enumerate(channels)}
        once = PlaneHistograms(channels, ranges, bins=64, joint=joint, joint_bins=16)
        once.update(blk.velocity, blk.pressure, scalar)
        cpu = {"u": blk.velocity[:, 0], "v": blk.velocity[:, 1], "w": blk.velocity[:, -1], "p": blk.pressure[:, 0],
               "T": None if scalar is None else scalar[:, 0]}
        fed = (once, [cpu[c].cpu().numpy().copy() for c in channels])
    outs.append(env.step(action))                        # no recorder is active any more
    state = (env._block.velocity.clone(), env._block.pressure.clone())
    sim_steps = env._n_sim_steps
    env.close()
    return outs, state, sim_steps, hist, stats, fed


@pytest.mark.parametrize("family", ("tcf", "rbc"))
def test_env_records_histograms_and_leaves_the_run_alone(family):
    _, _, _, channels, joint = ENVS[family]
    outs, state, sim_steps, hist, stats, (once, fields) = _env_run(family, True)
    assert hist.channels == channels and hist.n_samples == 2 * sim_steps
    nz, (ny, nx) = (state[0].shape[2] if family == "tcf" else 1), state[0].shape[-2:]
    total = hist._state()[0].sum(axis=-1)
    assert total.shape == (2, ny, len(channels)) and (total == hist.n_samples * nz * nx).all()
    pair = hist.joint_counts(*joint[0]).sum(axis=(-1, -2)) + hist.joint_outside(*joint[0])
    assert (pair == hist.n_samples * nz * nx).all()
    # every cell lies within half a bin of its bin's centre: the two means differ by at most that, where nothing fell outside
    rows_inside = 0
    for ch in channels:
        inside = (hist.below(ch) == 0) & (hist.above(ch) == 0) & (hist.nonfinite(ch) == 0)
        k = channels.index(ch)
        bound = 0.5 * hist.width(ch)[None] + 1e-6 * (hist.hi[:, k] - hist.lo[:, k])[None]
        diff = np.abs(hist.mean(ch) - stats.mean(ch))
        print(family, ch, "rows inside:", int(inside.sum()), "of", inside.size, "largest |mean difference| / bound:",
              float((diff / bound)[inside].max()) if inside.any() else None)
        assert (diff <= bound)[inside].all()
        rows_inside += int(inside.sum())
    assert rows_inside > 0                               # (the auto ranges, widened by half the span, hold two steps)
    # one sample of the block's tensors against the checker on copies of them
    fields4 = [f if f.ndim == 4 else f[:, None] for f in fields]
    want_c, want_j = ref.histogram(fields4, list(range(ny)), once.lo_real, once.scale, 64, once.pairs, 16)
    got_c, got_j = once._state()
    assert np.array_equal(got_c, want_c) and np.array_equal(got_j, want_j) and once.n_samples == 1
    # a run that never started a recorder: the same outputs while recording, and after the recorders stopped
    outs_off, state_off, _, _, _, _ = _env_run(family, False)
    _same(outs, outs_off)
    assert torch.equal(state[0], state_off[0]) and torch.equal(state[1], state_off[1])


def test_env_start_and_stop_guards():
    env = fluidgym_amd.make("RBC2D-easy-v0", **RBC)
    with pytest.raises(RuntimeError, match="reset"):
        env.start_flow_histograms()
    env.reset(seed=1)
    assert env._hook("flow_hist") is None
    with pytest.raises(RuntimeError, match="no histograms"):
        env.stop_flow_histograms()
    with pytest.raises(ValueError):
        env.start_flow_histograms(channels=("u", "w"))
    with pytest.raises(ValueError):
        env.start_flow_histograms(rows=[0, 999])
    ny = int(env._block.velocity.shape[-2])
    env.start_flow_histograms(ranges={"v": (-1.0, 1.0), "T": (0.0, 1.0)}, channels=("v", "T"), rows=[1, ny - 1], every=2, bins=16,
                              joint=(("v", "T"),), joint_bins=4)
    env.step(torch.zeros(2, 4, 1, device="cuda"))
    hist = env.stop_flow_histograms()
    assert env._hook("flow_hist") is None and hist.n_samples == env._n_sim_steps // 2 and hist.counts("T").shape == (2, 2, 16)
    with pytest.raises(RuntimeError, match="no histograms"):
        env.stop_flow_histograms()
    env.close()
