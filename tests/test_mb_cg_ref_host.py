"""The NumPy reference of the multi-block pressure CG (tests/mb_cg_ref.py) on the CPU, on the systems of tests/golden/mbc_forms.npz
with the neighbour tables of a host-only handle (device < 0, as tests/test_mb_tables.py): its operator is the dense matrix, its fp64
solve lands on the least-squares solution, and the bound the GPU forms are held to (tests/test_gpu_mb_cg_solutions.py) rejects a
solve whose x update is off by 2^-10 while its residual recurrence is right -- on every fixture mesh, before anything runs on a GPU."""
import numpy as np
import pytest

from tests import mb_cg_ref as R
from tests.test_gpu_mbc_forms import B, GOLDEN, MESHES
from tests.test_mb_tables import HostTables


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def tables():
    out = {}
    for mesh, fn in MESHES.items():
        t = HostTables(fn())
        out[mesh] = t.table(0, np.int32).reshape(2 * t.d, t.N).copy()
        t.close()
    return out


def _system(golden, tables, mesh, b):
    return golden[mesh + ".diag"][b], golden[mesh + ".off"][b], tables[mesh], golden[mesh + ".rhs"][b], golden[mesh + ".yp"]


@pytest.mark.parametrize("mesh", list(MESHES))
def test_apply_P_is_the_dense_matrix(mesh, golden, tables):
    diag, off, nbr, rhs, yp = _system(golden, tables, mesh, 1)
    N = diag.shape[0]
    assert nbr.shape == off.shape and (nbr < N).all()
    A = R.dense_P(diag, off, nbr)
    # built independently of apply_P's masks: entry by entry
    A2 = np.zeros((N, N))
    for i in range(N):
        A2[i, i] += float(diag[i])
        for f in range(nbr.shape[0]):
            if nbr[f, i] >= 0:
                A2[i, nbr[f, i]] += float(off[f, i])
    assert np.array_equal(A, A2)
    x = np.random.default_rng(3).standard_normal(N)
    y = R.apply_P(diag, off, nbr, x)
    # both are sums of at most 2d + 1 fp64 products per row, in another order
    assert np.abs(y - A @ x).max() <= 8 * np.finfo(np.float64).eps * (np.abs(A) @ np.abs(x)).max()
    # the criterion: the constant / the installed vector taken out of the residual
    for pm in (0, 1, 2):
        for dtype in (np.float32, np.float64):
            u = None if pm == 0 else (np.ones(N) if pm == 1 else yp.astype(np.float64))
            want = np.sqrt((x @ x - (0.0 if u is None else (u @ x) ** 2 / (u @ u))) / N)
            assert np.isclose(R.projected_rms(x, yp, pm, dtype), want, rtol=1e-6 if dtype is np.float32 else 1e-13)
            y = R.installed_vector(yp, pm, N, dtype)     # of length one to the rounding of its dtype, as the handle holds it
            if y is not None:
                assert y.dtype == dtype and abs(float(y.astype(np.float64) @ y.astype(np.float64)) - 1.0) < 8 * np.finfo(dtype).eps


@pytest.mark.parametrize("mesh", ["polar_ring", "channel40x30"])
def test_fp64_reference_lands_on_the_least_squares_solution(mesh, golden, tables):
    """pm = 1 solves the PROJECTED system Q P x = Q b, Q = I - 1 1^T / N: the matrix is fp32 words, symmetric and with zero row and
    column sums only to 1e-7, and the right-hand side has its mean removed in fp32, so b - P x keeps a constant component (1e-6) that
    the criterion ignores by construction -- the plain least-squares solution, which spreads that component over the smallest
    singular directions, is 1e-4 away and is not what the solver is after.  Against the least-squares solution x_q of the dense
    projected system, outside its null vector: Q P (x - x_q) = Q r_q - Q r_x, so |x - x_q| <= (|Q r_x| + |Q r_q|) / sigma_min+.
    That identity holds for any x, so |Q r_x| is not taken from the iterate but from what a converged solve may leave: it reports
    less than tol and its true residual is within 4 U of that, i.e. |Q r_x| <= sqrt(N) (tol + 4 U) -- a bound known before the
    solve ends (U from the largest iterate), plus the rounding of the dense solve itself (cap 5000, the fixture's fp64 tolerance)."""
    tol = float(golden["tol.f64"])
    eps = np.finfo(np.float64).eps
    for b in range(B):
        diag, off, nbr, rhs, yp = _system(golden, tables, mesh, b)
        N = diag.shape[0]
        x, reported, its, xmax = R.cg_reference(diag, off, nbr, rhs, yp, 1, tol, 5000, np.float64)
        assert reported < tol and 20 < its < 5000 and (xmax >= np.abs(x)).all()
        Q = np.eye(N) - np.full((N, N), 1.0 / N)
        A = R.dense_P(diag, off, nbr)
        Us, sv, Vt = np.linalg.svd(Q @ A)
        assert sv[-1] < 1e-12 * sv[0] and sv[-2] > 1e-5 * sv[0]      # one null vector, the rest well away from it
        qb = Q @ rhs.astype(np.float64)
        x_q = Vt[:-1].T @ ((Us[:, :-1].T @ qb) / sv[:-1])
        r_q, r_x = Q @ (rhs - A @ x_q), Q @ (rhs - A @ x)
        true = R.true_residual(diag, off, nbr, rhs, x, yp, 1, np.float64)
        assert np.isclose(true, np.linalg.norm(r_x) / np.sqrt(N), rtol=1e-9)
        err = np.linalg.norm((x - Vt[-1] * (Vt[-1] @ x)) - x_q)
        U = R.rounding_unit(diag, off, nbr, rhs, xmax, np.float64)
        bound = (np.sqrt(N) * (tol + R.GAP_FACTOR * U) + np.linalg.norm(r_q)) / sv[-2] + 64 * eps * (sv[0] / sv[-2]) * np.linalg.norm(x_q)
        print(f"MB_CG_REF_LS {mesh} env {b}: iterations {its} reported {reported:.3e} true {true:.3e} |x - x_q| {err:.3e} bound {bound:.3e}")
        assert abs(true - reported) <= R.GAP_FACTOR * U
        assert err <= bound


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("cap", [20, 40])
@pytest.mark.parametrize("mesh", list(MESHES))
def test_bound_rejects_an_x_update_off_by_2_to_the_minus_10(mesh, cap, dtype, golden, tables):
    """The teeth of the bound (fp32; and fp64, where the float word the residual is reported in is the larger part of it):
    x += alpha (1 + 2^-10) p with r -= alpha P p untouched, so the trajectory and the reported
    residual are those of the sound solve to the bit -- and the sound solve itself passes.  At the caps that end in front of the first
    restart: a restart rebuilds r = b - P x from the spoiled x, after which the recurrence residual carries the defect itself and
    the solve repairs it (what is left is 2^-10 of the residual at the last restart, below U once that is small) -- a defect in x is
    visible in the gap only up to the next restart, which is why the GPU test keeps the short caps."""
    tol = float(golden["tol.f32" if dtype is np.float32 else "tol.f64"])
    for b in range(B):
        diag, off, nbr, rhs, yp = _system(golden, tables, mesh, b)
        g_ref, U = R.gap_terms(diag, off, nbr, rhs, yp, 1, tol, cap, dtype)
        x, reported, its, _ = R.cg_reference(diag, off, nbr, rhs, yp, 1, tol, cap, dtype)
        tag = f"{mesh}.cap{cap}.{np.dtype(dtype).name} env {b}"
        R.check_solution("ref." + tag, diag, off, nbr, rhs, x, reported, reported < tol, yp, 1, tol, g_ref, U, dtype)
        xb, rep_b, its_b, _ = R.cg_reference(diag, off, nbr, rhs, yp, 1, tol, cap, dtype, x_alpha_scale=1.0 + 2.0 ** -10)
        assert rep_b == reported and its_b == its and not np.array_equal(xb, x)
        gap = abs(R.true_residual(diag, off, nbr, rhs, xb, yp, 1, dtype) - rep_b)
        assert gap > R.GAP_FACTOR * max(g_ref, U), (mesh, cap, b, gap, g_ref, U)      # the gap assertion itself, not a later one
        with pytest.raises(AssertionError):
            R.check_solution("spoiled." + tag, diag, off, nbr, rhs, xb, rep_b, rep_b < tol, yp, 1, tol, g_ref, U, dtype)
