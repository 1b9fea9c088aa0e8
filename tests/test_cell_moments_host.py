"""Per-cell flow statistics without a GPU: ``HostCellMoments`` against the reference's golden values and against a long-double
one-shot evaluation, merging and pooling, the files, ``span_average=False``, and the argument checks of ``fg_mb_cell_moments``."""
import ctypes
import os
import re

import numpy as np
import pytest

from fluidgym_amd import _lib as L
from fluidgym_amd.simulation.cell_moments import FILE_META, FILE_STATE, MAX_BLOCKS, CellMoments, HostCellMoments
from tests.cell_moments_ref import BOUND_GOLDEN, BOUND_ONE_SHOT, layout, make_fields, one_shot, worst_errors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_cell_moments.npz")
CASES = {"d2": (5, 3), "d3": (5, 3, 4)}                      # the golden blocks, (nx, ny[, nz])
SIZES_2D = [(5, 3), (4, 7), (1, 1)]
SIZES_3D = [(5, 3, 4), (2, 2, 1), (3, 1, 7)]


def _flat(g, tag, s):
    """Sample ``s`` of a golden block as the flat fields of a one-block domain: velocity [1, d, N], pressure [1, N]."""
    u, p = g[f"{tag}_velocity"][s], g[f"{tag}_pressure"][s]
    return u.reshape(1, u.shape[1], -1), p.reshape(1, -1)


def _golden_record(g, tag):
    acc = HostCellMoments([(CASES[tag], 0)], len(CASES[tag]))
    fields = [_flat(g, tag, s) for s in range(3)]
    for u, p in fields:
        acc.update(u, p)
    return acc, fields


def _run(sizes, fields, span_average=True):
    acc = HostCellMoments(layout(sizes)[0], len(sizes[0]), span_average)
    for u, p in fields:
        acc.update(u, p)
    return acc


def _golden_pairs(g, tag, acc):
    """Golden key -> (ours, scale) in the shape of the golden array: means against abs1 / n, sums against absM."""
    d = acc.dims
    n, _, _, abs1, absM = one_shot(acc, [_flat(g, tag, s) for s in range(3)])
    mean = lambda ks: np.stack([acc.mean(k, 0)[0] for k in ks])
    mscale = lambda ks: np.stack([acc._block(np.asarray(abs1[:, k] / n, np.float64), 0)[0] for k in ks])
    raw = lambda ps: np.stack([acc.covariance(i, j, 0)[0] * acc.n(0) for i, j in ps])
    cscale = lambda ps: np.stack([acc._block(np.asarray(absM[:, acc._pair(i, j)], np.float64), 0)[0] for i, j in ps])
    vel = list(range(d))
    out = {f"{tag}_vel_mean": (mean(vel), mscale(vel)), f"{tag}_vel_sum_squares": (raw([(k, k) for k in vel]), cscale([(k, k) for k in vel])),
           f"{tag}_p_mean": (mean([d]), mscale([d])), f"{tag}_p_sum_squares": (raw([(d, d)]), cscale([(d, d)]))}
    for a in range(d):
        for b in range(a + 1, d):
            ab = "uvw"[a] + "uvw"[b]
            out.update({f"{tag}_cov_{ab}_mean_x": (mean([a]), mscale([a])), f"{tag}_cov_{ab}_mean_y": (mean([b]), mscale([b])),
                        f"{tag}_cov_{ab}_C": (raw([(a, b)]), cscale([(a, b)]))})
    return out


@pytest.mark.parametrize("tag", list(CASES))
def test_host_twin_equals_the_reference_golden_values(tag):
    g = np.load(GOLDEN)
    acc, _ = _golden_record(g, tag)
    nz = CASES[tag][2] if tag == "d3" else 1
    assert acc.samples == 3 and acc.n(0) == 3.0 * nz
    assert acc.n(0) == float(g[f"{tag}_vel_n"]) == float(g[f"{tag}_p_n"]) == float(g[f"{tag}_cov_uv_n"])
    assert acc.mean("u", 0).shape == (1, 3, 5)
    pairs = _golden_pairs(g, tag, acc)
    assert set(pairs) == {k for k in g.files if k.startswith(tag) and k.rsplit("_", 1)[1] not in ("velocity", "pressure", "n", "welford", "covariance")}
    worst = max(float(np.max(np.abs(ours - g[key]) / scale)) for key, (ours, scale) in pairs.items())
    print(f"{tag}: worst error against the golden values / absolute-monomial sum: {worst:.2e}")
    assert worst <= BOUND_GOLDEN
    assert np.array_equal(acc.variance("v", 0), acc.covariance("v", "v", 0)) and np.array_equal(acc.covariance(0, 1, 0), acc.covariance("v", "u", 0))
    vel = range(acc.dims)
    assert np.allclose(acc.tke(0), 0.5 * sum(acc.variance(k, 0) for k in vel), rtol=1e-15)


@pytest.mark.parametrize("sizes", [SIZES_2D, SIZES_3D], ids=["2d", "3d"])
def test_merged_samples_merge_and_pooled_equal_the_one_shot(sizes):
    fields = make_fields(sizes, B=3, samples=4, seed=11, dtype=np.float64)
    acc = _run(sizes, fields)
    em, ec = worst_errors(acc, one_shot(acc, fields))
    print(f"mean {em:.2e}, central {ec:.2e} of the absolute-monomial sum")
    assert em <= BOUND_ONE_SHOT and ec <= BOUND_ONE_SHOT
    pm, pc = worst_errors(acc.pooled(), one_shot(acc, fields, pool_envs=True))
    print(f"pooled: mean {pm:.2e}, central {pc:.2e}")
    assert pm <= BOUND_ONE_SHOT and pc <= BOUND_ONE_SHOT and acc.pooled().samples == 12
    a, b = _run(sizes, fields[:1]), _run(sizes, fields[1:])
    mm, mc = worst_errors(a.merge(b), one_shot(acc, fields))             # disjoint samples: the record of all of them
    assert mm <= BOUND_ONE_SHOT and mc <= BOUND_ONE_SHOT and a.samples == 4
    empty = HostCellMoments(layout(sizes)[0], len(sizes[0]))
    assert empty.merge(b).samples == 3 and np.array_equal(empty._state()[0], b._state()[0])
    with pytest.raises(ValueError, match="same blocks"):
        a.merge(_run(sizes[:2], make_fields(sizes[:2], B=3, dtype=np.float64)))


def test_accessors_shapes_and_at_cells():
    fields = make_fields(SIZES_3D, B=2, seed=3, dtype=np.float64)
    acc = _run(SIZES_3D, fields)
    assert [acc.mean("w", i).shape for i in range(3)] == [(2, 3, 5), (2, 2, 2), (2, 1, 3)]
    assert [acc.n(i) for i in range(3)] == [12.0, 3.0, 21.0] and acc.NC == 15 + 4 + 3
    assert acc.flat("mean", "p").shape == (2, 22) and np.array_equal(acc.flat("n")[1], np.repeat([12.0, 3.0, 21.0], [15, 4, 3]))
    assert np.array_equal(acc.mean("p", 1), acc.flat("mean", "p")[:, 15:19].reshape(2, 2, 2))
    m, v = acc.at_cells("p", [21, 0, 16])
    assert m.shape == v.shape == (2, 3) and np.array_equal(m[:, 2], acc.mean("p", 1)[:, 0, 1]) and np.array_equal(v[:, 0], acc.variance("p", 2)[:, 0, 2])
    with pytest.raises(IndexError):
        acc.at_cells("p", [22])
    with pytest.raises(KeyError):
        acc.flat("skewness", "u")
    with pytest.raises(RuntimeError, match="no sample"):
        HostCellMoments([((2, 2), 0)], 2).mean("u", 0)
    with pytest.raises(ValueError):
        HostCellMoments([((2, 2), 0)] * (MAX_BLOCKS + 1), 2)
    with pytest.raises(ValueError):
        HostCellMoments([((2, 2, 2), 0)], 2)
    with pytest.raises(ValueError, match="flat multi-block"):
        acc.update(np.zeros((2, 3, 4, 5)), np.zeros((2, 20)))
    with pytest.raises(ValueError, match="GPU"):
        CellMoments(layout(SIZES_3D)[0], 3).update(*fields[0])


def test_a_non_finite_cell_poisons_its_column_only():
    fields = make_fields(SIZES_3D, B=2, seed=5, dtype=np.float64)
    clean = _run(SIZES_3D, fields)
    fields[1][0][1, 2, 2 * 15 + 7] = np.inf                  # sample 1, env 1, channel w, block 0, z 2, column 7
    dirty = _run(SIZES_3D, fields)
    bad = np.zeros((2, 22), bool)
    bad[1, 7] = True
    for a, b in zip(clean._state(), dirty._state()):
        a, b = np.moveaxis(a, 1, 2), np.moveaxis(b, 1, 2)
        assert np.isnan(b[bad]).all() and np.array_equal(a[~bad], b[~bad])


def test_span_average_off_treats_every_cell_as_a_column():
    sizes = [(5, 3, 4)]
    fields = make_fields(sizes, B=2, seed=9, dtype=np.float64)
    cells = _run(sizes, fields, span_average=False)
    as_columns = _run([(5, 12, 1)], fields)                 # the same cells as 60 columns of one cell each
    assert cells.n(0) == 3.0 and cells.NC == 60 and cells.mean("u", 0).shape == (2, 4, 3, 5)
    for a, b in zip(cells._state(), as_columns._state()):
        assert a.tobytes() == b.tobytes()
    em, ec = worst_errors(cells, one_shot(cells, fields))
    assert em <= BOUND_ONE_SHOT and ec <= BOUND_ONE_SHOT
    # equal weights: the span average of the per-cell means is the mean of the columns
    spanned = _run(sizes, fields)
    assert np.allclose(cells.mean("p", 0).mean(axis=1), spanned.mean("p", 0), rtol=0, atol=1e-12 * np.abs(spanned.mean("p", 0)).max())


@pytest.mark.parametrize("tag", list(CASES))
def test_save_load_round_trip_and_the_reference_layouts(tag, tmp_path):
    g = np.load(GOLDEN)
    acc, _ = _golden_record(g, tag)
    acc.save(tmp_path / "gold")
    d = tmp_path / "gold" / "env_0000"
    pairs = ["uv"] + (["uw", "vw"] if tag == "d3" else [])
    names = ["block0_vel_stats.npz", "block0_p_stats.npz"] + [f"block0_vel_cov_{ab}.npz" for ab in pairs]
    assert sorted(os.listdir(d)) == sorted(names + [FILE_STATE]) and os.path.exists(tmp_path / "gold" / FILE_META)
    worst = 0.0
    scales = _golden_pairs(g, tag, acc)
    for name, prefix, keys in [(names[0], f"{tag}_vel_", "keys_welford"), (names[1], f"{tag}_p_", "keys_welford")] + \
                              [(f"block0_vel_cov_{ab}.npz", f"{tag}_cov_{ab}_", "keys_covariance") for ab in pairs]:
        with np.load(d / name) as z:
            assert sorted(z.keys()) == list(g[f"{tag}_{keys}"]), (name, sorted(z.keys()))
            for key in z.keys():
                ref = g[prefix + key]
                assert z[key].shape == ref.shape and z[key].dtype == ref.dtype, (name, key, z[key].shape, ref.shape)
                if key == "n":
                    assert z[key] == ref
                else:       # the file holds the golden numbers, at the bound of the comparison with the record itself
                    worst = max(worst, float(np.max(np.abs(z[key] - ref) / scales[prefix + key][1])))
    print(f"{tag}: worst difference between a saved file and the golden values / absolute-monomial sum: {worst:.2e}")
    assert worst <= BOUND_GOLDEN
    back = HostCellMoments.load(tmp_path / "gold")
    assert back.samples == 3 and back.blocks == acc.blocks and back.span_average
    for a, b in zip(acc._state(), back._state()):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_save_per_env_pooled_and_without_span_average(tmp_path):
    fields = make_fields(SIZES_3D, B=3, seed=7, dtype=np.float64)
    acc = _run(SIZES_3D, fields)
    acc.save(tmp_path / "per_env")
    acc.save(tmp_path / "pooled", pooled=True)
    assert sorted(p for p in os.listdir(tmp_path / "per_env")) == ["cell_moments.json", "env_0000", "env_0001", "env_0002"]
    back = HostCellMoments.load(tmp_path / "per_env")
    for a, b in zip(acc._state(), back._state()):
        assert a.tobytes() == b.tobytes()
    pooled = HostCellMoments.load(tmp_path / "pooled")
    assert pooled.samples == 9
    for a, b in zip(acc.pooled()._state(), pooled._state()):
        assert a.tobytes() == b.tobytes()
    with np.load(tmp_path / "per_env" / "env_0001" / "block2_vel_stats.npz") as z:
        assert z["n"] == 21 and z["mean"].shape == (3, 1, 3) and np.array_equal(z["mean"][2], acc.mean("w", 2)[1])
        assert np.allclose(z["sum_squares"][1], acc.variance("v", 2)[1] * 21, rtol=1e-14, atol=0)
    with np.load(tmp_path / "pooled" / "block1_vel_cov_vw.npz") as z:
        assert z["n"] == 9 and np.allclose(z["C"][0], acc.pooled().covariance("v", "w", 1)[0] * 9, rtol=1e-14, atol=0)
    cells = _run(SIZES_3D, fields, span_average=False)
    cells.save(tmp_path / "cells", pooled=True)
    with np.load(tmp_path / "cells" / "block0_p_stats.npz") as z:     # dims = [0] on a 3-D block: [1, nz, ny, nx]
        assert z["n"] == 9 and z["mean"].shape == (1, 4, 3, 5)
    assert not HostCellMoments.load(tmp_path / "cells").span_average


def test_cell_moments_abi_and_argument_checks():
    """The argument checks return before anything touches the device: the pointers here are never read."""
    header = open(os.path.join(ROOT, "include", "fluidgym_hip.h")).read()
    assert re.search(r"\bint\s+fg_mb_cell_moments\s*\(", header)
    assert "fg_mb_cell_moments" in L.SIGNATURES and "fg_mb_cell_moments" in L.SIGNATURES_F64
    mk = open(os.path.join(ROOT, "fluidgym_amd", "csrc", "Makefile")).read()
    assert all("fg_cellstats.hip" in line for line in mk.splitlines() if line.startswith(("SRCS =", "F64_SRCS =")))
    one = ctypes.c_void_p(64)
    table = lambda rows: (ctypes.c_int64 * (4 * len(rows)))(*[v for r in rows for v in r])
    ok = table([(0, 15, 1, 0), (15, 28, 1, 15)])
    for lib in (L.load(), L.load_f64()):
        f = lib.fg_mb_cell_moments
        bad = [
            (None, one, 2, 1, 43, ok, 2, 0, one, one),                               # null pointers
            (one, None, 2, 1, 43, ok, 2, 0, one, one),
            (one, one, 2, 1, 43, None, 2, 0, one, one),
            (one, one, 2, 1, 43, ok, 2, 0, None, one),                               # null accumulators
            (one, one, 2, 1, 43, ok, 2, 0, one, None),
            (one, one, 1, 1, 43, ok, 2, 0, one, one),                                # dims outside 2..3
            (one, one, 4, 1, 43, ok, 2, 0, one, one),
            (one, one, 2, 0, 43, ok, 2, 0, one, one),                                # batch, n_cells, n_blocks, samples
            (one, one, 2, 1, 0, ok, 2, 0, one, one),
            (one, one, 2, 1, 43, ok, 0, 0, one, one),
            (one, one, 2, 1, 43, table([(i, 1, 1, i) for i in range(9)]), 9, 0, one, one),       # more blocks than the table holds
            (one, one, 2, 1, 43, ok, 2, -1, one, one),
            (one, one, 2, 1, 42, ok, 2, 0, one, one),                                # the last block ends past the field
            (one, one, 2, 1, 43, table([(-1, 15, 1, 0)]), 1, 0, one, one),
            (one, one, 2, 1, 43, table([(2 ** 63 - 8, 15, 1, 0)]), 1, 0, one, one),  # an offset whose end wraps around
            (one, one, 3, 1, 2 ** 31 - 1, table([(0, 2 ** 31 - 1, 2 ** 31 - 1, 0)]), 1, 0, one, one),
            (one, one, 2, 1, 43, table([(0, 0, 1, 0)]), 1, 0, one, one),             # non-positive extents
            (one, one, 3, 1, 43, table([(0, 5, 0, 0)]), 1, 0, one, one),
            (one, one, 3, 1, 43, table([(0, 5, 9, 0)]), 1, 0, one, one),             # 45 cells in a field of 43
            (one, one, 2, 1, 43, table([(0, 15, 1, 0), (15, 28, 1, 16)]), 2, 0, one, one),       # column_offset is not the running sum
        ]
        for args in bad:
            assert f(*args, None) == -1, args
            assert b"fg_mb_cell_moments" in lib.fg_last_error()


def test_the_planned_load_form_per_block():
    """``fg_mb_cell_moments_widths`` runs the launch's own plan on the host: 16-byte loads where the pointers, N, NC and the block's first
    cell, layer and first column allow, per block."""
    table = lambda rows: (ctypes.c_int64 * (4 * len(rows)))(*[v for r in rows for v in r])
    mixed = [(0, 32, 1, 0), (32, 15, 1, 32), (47, 1, 1, 47), (48, 16, 1, 48)]          # N = NC = 64
    spans = [(0, 32, 4, 0), (128, 16, 2, 32)]                                          # N = 160, NC = 48
    odd = [(0, 15, 1, 0), (15, 28, 1, 15), (43, 1, 1, 43)]                             # N = NC = 44
    for lib, vec in ((L.load(), 4), (L.load_f64(), 2)):
        def widths(rows, n_cells, u=4096, p=8192, m=16384, c=32768):
            out = (ctypes.c_int32 * len(rows))()
            rc = lib.fg_mb_cell_moments_widths(ctypes.c_void_p(u), ctypes.c_void_p(p), n_cells, table(rows), len(rows), ctypes.c_void_p(m),
                                               ctypes.c_void_p(c), out)
            assert rc == 0, lib.fg_last_error()
            return list(out)
        assert widths(mixed, 64) == [vec, 1, 1, vec] and widths(spans, 160) == [vec, vec] and widths(odd, 44) == [1, 1, 1]
        for unaligned in (dict(u=4096 + 8), dict(p=8192 + 8), dict(m=16384 + 8), dict(c=32768 + 8)):
            assert widths(mixed, 64, **unaligned) == [1, 1, 1, 1]
        assert widths(mixed, 65) == [1, 1, 1, 1] and widths(mixed[:2], 64) == [1, 1]         # N, NC (47) not multiples of the vector
        assert lib.fg_mb_cell_moments_widths(ctypes.c_void_p(64), ctypes.c_void_p(64), 64, table(mixed), 4, ctypes.c_void_p(64),
                                             ctypes.c_void_p(64), None) == -1
        assert lib.fg_mb_cell_moments_widths(ctypes.c_void_p(64), ctypes.c_void_p(64), 63, table(mixed), 4, ctypes.c_void_p(64),
                                             ctypes.c_void_p(64), (ctypes.c_int32 * 4)()) == -1
