"""Plain NumPy restatement of the multi-block pressure CG (``csrc/fg_mb_krylov.hip::mb_cg``) and of the quantities its iterate x is
held to (tests/test_mb_cg_ref_host.py on the CPU, tests/test_gpu_mb_cg_solutions.py on the GPU).  One system at a time, in the layout
the kernels read: ``diag [N]``, ``off [F][N]``, ``nbr [F][N]`` from ``Domain.neighbors()`` (negative = a prescribed face, no entry).

What a solve REPORTS is the recurrence residual: r is updated as r -= alpha P p, independently of x += alpha p, so a wrong x update
leaves the report untouched.  What it is held to is the residual of its x, evaluated in fp64:

    true     = projected_rms(b - apply_P(x), yp, pm)       yp: the direction the handle projects out, at length one
    U        = eps(dtype) * rms(|P| max_k|x_k| + |b|)     the rounding unit of ONE residual evaluation at the largest iterate
    g_ref    = |true - reported| of ``cg_reference`` on the same system, cap and dtype (reported through the ABI's float word)
    bound    : |true - reported| <= GAP_FACTOR * max(g_ref, U)

The gap between recurrence and true residual is what the rounding of every x and r update has accumulated (Greenbaum 1997: a sum
over the iterations of terms eps |P| |x_k|); it depends on the trajectory, so it is measured on the reference's own trajectory rather
than modelled, with U as its floor (a short or lucky solve can leave the reference a gap below one rounding of the evaluation).  The
forms differ from the reference in the summation order of their dot products (workgroup trees into exact accumulators against a
sequential fp64 dot) and in which products -ffp-contract=fast fuses: a small factor, GAP_FACTOR = 4, not an order of magnitude.
``max_k|x_k|`` is the element-wise maximum over the iterates of the reference run."""
import numpy as np

GAP_FACTOR = 4.0
CHUNK, RESTART = 20, 100      # MB_CG_CHUNK, MB_CG_RESTART (csrc/fg_mb_solve.h)


def apply_P(diag, off, nbr, x):
    """diag * x + sum_f off[f] * x[nbr[f]] over the faces with a neighbour, in fp64."""
    x = np.asarray(x, np.float64)
    y = np.asarray(diag, np.float64) * x
    for f in range(nbr.shape[0]):
        m = nbr[f] >= 0
        y[m] += np.asarray(off[f], np.float64)[m] * x[nbr[f][m]]
    return y


def dense_P(diag, off, nbr):
    N = diag.shape[0]
    A = np.zeros((N, N))
    A[np.arange(N), np.arange(N)] = np.asarray(diag, np.float64)
    for f in range(nbr.shape[0]):
        m = np.nonzero(nbr[f] >= 0)[0]
        np.add.at(A, (m, nbr[f][m]), np.asarray(off[f], np.float64)[m])
    return A


def installed_vector(yp, pm, N, dtype):
    """The vector the kernels project out, as the handle holds it in ``dtype``: none (pm 0), the constant (1) or ``yp`` (2), scaled
    to unit length in ``dtype`` by fg_mb_set_residual_projection -- so of length one only to the rounding of ``dtype``."""
    if pm == 0:
        return None
    T = np.dtype(dtype).type
    y = np.ones(N, T) if pm == 1 else np.asarray(yp, T)
    return y * T(1.0 / np.sqrt(float(y.astype(np.float64) @ y.astype(np.float64))))


def unit_vector(yp, pm, N, dtype):
    """The direction of the installed vector at length one in fp64: what the true residual is projected along (for pm 1 the constant
    unit vector).  The fixture's yp itself is not it: the handle rescales what it is given."""
    y = installed_vector(yp, pm, N, dtype)
    if y is None:
        return None
    y = y.astype(np.float64)
    return y / np.sqrt(y @ y)


def projected_rms(r, yp, pm, dtype=np.float64):
    """sqrt((|r|^2 - (yp.r)^2) / N), yp of length one: the criterion of mbc_ap_head / k_mbs_check."""
    r = np.asarray(r, np.float64)
    y = unit_vector(yp, pm, r.size, dtype)
    c = 0.0 if y is None else float(y @ r)
    return float(np.sqrt(max(float(r @ r) - c * c, 0.0) / r.size))


def true_residual(diag, off, nbr, rhs, x, yp, pm, dtype):
    return projected_rms(np.asarray(rhs, np.float64) - apply_P(diag, off, nbr, x), yp, pm, dtype)


def rounding_unit(diag, off, nbr, rhs, xmax, dtype):
    v = apply_P(np.abs(np.asarray(diag, np.float64)), np.abs(np.asarray(off, np.float64)), nbr, xmax) + np.abs(np.asarray(rhs, np.float64))
    return float(np.finfo(dtype).eps * np.sqrt(np.mean(v * v)))


def _spmv(diag, off, nbr, safe, v):
    """P v with every product and sum in the dtype of the vectors (safe = nbr with the prescribed faces pointed at cell 0, off = 0 there)."""
    y = diag * v
    for f in range(nbr.shape[0]):
        y = y + off[f] * v[safe[f]]
    return y


def _word(crit):
    """The residual as a solve reports it: ``fg_solve_info.final_residual`` is a float in both libraries, so the fp64 one rounds its
    criterion to fp32 on the way out (2^-24 of it: 1e-8 of an unconverged 0.2, 1e-19 of a converged 1e-12).  The reference reports
    through the same word, which puts that rounding into g_ref instead of into the factor of the bound."""
    return float(np.float32(crit))


def cg_reference(diag, off, nbr, rhs, yp, pm, tol, cap, dtype, stall_limit=400, x_alpha_scale=1.0):
    """mb_cg's recurrence from x = 0 with vectors in ``dtype`` and dot products in fp64: the criterion is the projected RMS of the
    recurrence residual, the direction is built on the projected residual, r = b - P x and p = r again every RESTART iterations, the
    verdicts fall where the kernels take them (every iteration's head for "converged", every CHUNK iterations for the cap -- rounded
    up to whole chunks -- and the stall limit), x_it is kept when its criterion halves the kept one and handed back, with its
    criterion and iteration, when the solve ends unconverged -- or breaks down: a criterion that is not finite (on a non-symmetric
    matrix r ends up almost constant and |r|^2 - (yp.r)^2 cancels to below zero) sends the kernels back to the kept iterate, too;
    their retry from a restart while iterations are left is not restated, the solve ends there.
    Returns (x, reported residual, iterations, max_k |x_k| per cell).
    ``x_alpha_scale`` != 1 spoils the x update alone (r is updated correctly): the defect the bound has to catch."""
    T = np.dtype(dtype).type
    N = diag.shape[0]
    diag, rhs = np.asarray(diag, T), np.asarray(rhs, T)
    off = np.where(nbr >= 0, np.asarray(off, T), T(0))
    safe = np.maximum(nbr, 0)
    yT = installed_vector(yp, pm, N, T)
    d64 = lambda a, b: a.astype(np.float64) @ b.astype(np.float64)   # (np.float64: a zero divisor gives inf / nan, as on the GPU)
    with np.errstate(invalid="ignore", divide="ignore"):
        return _cg(T, N, diag, off, nbr, safe, rhs, yT, d64, tol, cap, stall_limit, x_alpha_scale)


def _cg(T, N, diag, off, nbr, safe, rhs, yT, d64, tol, cap, stall_limit, x_alpha_scale):
    tolT, max_it = T(tol), -(-int(cap) // CHUNK) * CHUNK
    x, r = np.zeros(N, T), rhs.copy()
    xmax = np.zeros(N)
    rho, sr = d64(r, r), (np.float64(0) if yT is None else d64(r, yT))
    best_x, best_crit, best_it = x.copy(), None, 0
    p, prev, it, fresh_at = None, np.float64(1), 0, 0
    while True:
        if it > 0 and it % CHUNK == 0:      # k_mbs_check behind a chunk, then the restart in front of the next one
            crit = T(np.sqrt((rho - sr * sr) / N))
            if not crit >= tolT and np.isfinite(crit):
                return x, _word(crit), it, xmax
            if not np.isfinite(crit) or it >= max_it or (stall_limit > 0 and it - 1 - best_it > stall_limit):
                return best_x, _word(best_crit), best_it, xmax
            if it % RESTART == 0:
                r = rhs - _spmv(diag, off, nbr, safe, x)
                rho, sr = d64(r, r), (np.float64(0) if yT is None else d64(r, yT))
                fresh_at = it
        proj = rho - sr * sr
        crit = T(np.sqrt(proj / N))
        if not np.isfinite(crit):
            return best_x, _word(best_crit), best_it, xmax
        if not crit >= tolT:
            return x, _word(crit), it, xmax
        if it == 0 or crit < T(0.5) * best_crit:
            best_x, best_crit, best_it = x.copy(), crit, it
        base = r if yT is None else r - T(sr) * yT
        p = base if it == fresh_at else base + T(proj / prev) * p
        v = _spmv(diag, off, nbr, safe, p)
        alpha = T(proj / d64(p, v))
        x = x + T(alpha * T(x_alpha_scale)) * p
        r = r - alpha * v
        np.maximum(xmax, np.abs(x), out=xmax)
        prev, rho, sr = proj, d64(r, r), (np.float64(0) if yT is None else d64(r, yT))
        it += 1


def gap_terms(diag, off, nbr, rhs, yp, pm, tol, cap, dtype, stall_limit=400):
    """(g_ref, U) of one system: the reference's own |true - reported| and the rounding unit at its largest iterate."""
    x, reported, _, xmax = cg_reference(diag, off, nbr, rhs, yp, pm, tol, cap, dtype, stall_limit)
    g_ref = abs(true_residual(diag, off, nbr, rhs, x, yp, pm, dtype) - reported)
    return g_ref, rounding_unit(diag, off, nbr, rhs, xmax, dtype)


def check_solution(label, diag, off, nbr, rhs, x, reported, converged, yp, pm, tol, g_ref, U, dtype):
    """The assertions every solve is held to; prints the record line first.  Returns |true - reported| / max(g_ref, U)."""
    true = true_residual(diag, off, nbr, rhs, x, yp, pm, dtype)
    slack = GAP_FACTOR * max(g_ref, U)
    ratio = abs(true - reported) / max(g_ref, U)
    print(f"MB_CG_TRUE_RES {label}: reported {reported:.6e} true {true:.6e} g_ref {g_ref:.3e} U {U:.3e} ratio {ratio:.3f}")
    assert np.isfinite(x).all(), label
    assert abs(true - reported) <= slack, (label, "true", true, "reported", reported, "g_ref", g_ref, "U", U)
    if converged:
        assert true <= tol + slack, (label, "true", true, "tol", tol, "g_ref", g_ref, "U", U)
    return ratio
