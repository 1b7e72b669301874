"""The yardstick of the tests of slod_lod_solve_multi_precond and slod_lod_solve_ensemble_precond (a plain module like
lod_cases.py): preconditioned CG in dense float64 numpy with the stop rule checked in every iteration on the recursive
residual, the Jacobi-preconditioned instance, and the bracket the GPU's iteration counts must lie in.  Nothing here calls
the library, so test_lod_pcg_reference.py checks it on the CPU.

The bracket: at rel_tol = tau the count of an implementation that rounds differently (fma, summation order, the banded
factor in place of a dense solve) lies between the reference's count at 10 tau and its count at tau / 10.  It is only
meaningful when those two are close: BRACKET_CAP = 3."""
import numpy as np

BRACKET_CAP = 3


def pcg_reference(A, solve_P, b, tol, max_it):
    """CG on A u = b from u = 0 with z = solve_P(r).  The count is the number of iterations after which
    r.r <= tol^2 b.b first holds (0 for b = 0), or max_it.  Returns (u, count, [||r_k|| / ||b||, k = 0 .. count])."""
    b = np.asarray(b, dtype=np.float64)
    u, r = np.zeros_like(b), b.copy()
    rhs2 = float(b @ b)
    rr = rhs2
    hist = [1.0 if rhs2 > 0.0 else 0.0]
    if rr <= tol * tol * rhs2:
        return u, 0, hist
    p = rz = None
    for it in range(1, max_it + 1):
        z = solve_P(r)
        rz_new = float(r @ z)
        p = z if p is None else z + (rz_new / rz if rz != 0.0 else 0.0) * p
        rz = rz_new
        Ap = A @ p
        pAp = float(p @ Ap)
        alpha = rz / pAp if pAp != 0.0 else 0.0
        u = u + alpha * p
        r = r - alpha * Ap
        rr = float(r @ r)
        hist.append(float(np.sqrt(rr / rhs2)))
        if rr <= tol * tol * rhs2:
            return u, it, hist
    return u, max_it, hist


def jacobi_reference(A, b, tol, max_it):
    """pcg_reference with z = D^-1 r, the recurrence of slod_lod_solve_multi."""
    d = np.diag(A).copy()
    d[d == 0.0] = 1.0
    return pcg_reference(A, lambda r: r / d, b, tol, max_it)


def dense_solver(P):
    """solve_P of a dense symmetric positive definite P (Cholesky once)."""
    import scipy.linalg as sl
    c = sl.cho_factor(P)
    return lambda r: sl.cho_solve(c, r)


def bracket(A, solve_P, b, tau, max_it=500):
    """(count at 10 tau, count at tau / 10, true relative residual of the reference at tau)."""
    _, lo, _ = pcg_reference(A, solve_P, b, 10.0 * tau, max_it)
    _, hi, _ = pcg_reference(A, solve_P, b, tau / 10.0, max_it)
    u, _, _ = pcg_reference(A, solve_P, b, tau, max_it)
    nb = np.linalg.norm(b)
    return lo, hi, float(np.linalg.norm(b - A @ u) / nb) if nb > 0.0 else 0.0


def check_bracket(label, got, lo, hi):
    """The cap first (a wide bracket asserts nothing), then the count."""
    assert hi - lo <= BRACKET_CAP, "%s: the reference's own counts %d .. %d are too far apart" % (label, lo, hi)
    assert lo <= got <= hi, "%s: %d iterations, the reference brackets %d .. %d" % (label, got, lo, hi)


def doubled_diagonal(A, rows):
    """A + sum_{i in rows} a_ii e_i e_i^T: the perturbation of rank len(rows) of the rank-bound tests."""
    out = A.copy()
    for i in rows:
        out[i, i] = 2.0 * A[i, i]
    return out


def few_mode_load(A, P, m=5):
    """A load on which CG for A preconditioned by P ends after m iterations in exact arithmetic, however far P is from A:
    b = P (w_1 + .. + w_m) with m eigenvectors of A w = lambda P w spread evenly over the spectrum (scaled to unit
    maximum), so that P^-1 b lies in an invariant subspace of P^-1 A of dimension m.  The residual then falls to rounding
    level in the last step, which keeps the counts at 10 tau and tau / 10 together where a general load on a far
    preconditioner converges by half a digit per iteration."""
    import scipy.linalg as sl
    lam, W = sl.eigh(A, P)
    idx = np.linspace(0, len(lam) - 1, m).round().astype(int)
    b = P @ W[:, idx].sum(axis=1)
    return b / np.abs(b).max()
