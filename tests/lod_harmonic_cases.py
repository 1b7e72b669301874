"""Helpers of the tests of the frequency response on the LOD space (slod_lod_factor_create_zldl,
slod_lod_factor_solve_complex, slod_lod_harmonic_response); a plain module like lod_ldl_cases.py, whose cases and bound
it shares.

The yardstick is an unpivoted complex LDL^T (plain transpose) in numpy complex128 of the dense
S = alpha A + beta M in factor order: L, d, the first bad pivot, G = || |L| |D| |L^T| ||_inf and ||S||_inf.  The modal
response from scipy's eigh(A, M), its eigenvalues polished by polished_spectrum, is the second, independent reference.  Nothing in the yardstick, the modal sum or the
sweep rule calls the library, so test_lod_harmonic_reference.py checks them on the CPU.

The sweep rule, per case (lam the ascending spectrum of (sym A, M), n its length): eight frequencies,
  sqrt(lam_1), sqrt(lam_2), sqrt(lam_{n/4}), sqrt(lam_{n/2}), sqrt(lam_n)     exactly on resonance
  sqrt(lam_1) / 2,  (sqrt(lam_3) + sqrt(lam_4)) / 2,  2 sqrt(lam_n)           off resonance
at three dampings: mass only dm = 0.02 sqrt(lam_1); stiffness only ds = 1e-3 / sqrt(lam_1); both.
The growth cap is a condition, not a measurement: before the library is called, every (damping, omega) must have a
yardstick without a bad pivot and with growth <= GROWTH_CAP; a frequency that fails is moved up by factors of 1 + 1/64, at
most 8 times (as shift_at moves a shift); none qualifies: AssertionError with the growths seen.

Bars (b = half bandwidth, u = 2^-53):
  norm_matrix     (2 b + 2) u relative;  norm_factor: a factor of 2 of G;  range of |D|: 1e-10 relative
  backward error  eta = ||b - S x||_inf / (G ||x||_inf + ||b||_inf) <= 4 sqrt(2) bound(b), the residual in np.clongdouble:
                  4 sqrt(2) u is Higham's constant of a complex division in the place of u of the real bound
  forward error   1e-8 of max |u| against numpy.linalg.solve and against the modal response
"""
import numpy as np

from lod_ldl_cases import CASES, GROWTH_CAP, U, bound, ldl_case, ldl_reference, q1_pencil   # noqa: F401

ZBOUND = 4.0 * np.sqrt(2.0)
FORWARD = 1e-8
MOVE, MOVES = 1.0 + 1.0 / 64.0, 8


class ZLdl:
    pass


def zldl_reference(S):
    """Unpivoted complex L D L^T (plain transpose) of the symmetric matrix whose lower triangle is that of S (already in
    factor order).  .L, .d, .bad (the first pivot with both parts zero or a part not finite; -1: none), .G, .norm."""
    n = S.shape[0]
    low = np.tril(S).astype(np.complex128)
    full = low + np.tril(low, -1).T
    W = full.copy()
    out = ZLdl()
    out.L, out.d, out.bad = np.eye(n, dtype=np.complex128), np.zeros(n, dtype=np.complex128), -1
    with np.errstate(all="ignore"):
        for j in range(n):
            p = out.d[j] = W[j, j]
            if not (np.isfinite(p.real) and np.isfinite(p.imag) and p != 0.0):
                out.bad = j
                break
            w = W[j + 1:, j].copy()
            out.L[j + 1:, j] = w / p
            W[j + 1:, j + 1:] -= np.outer(out.L[j + 1:, j], w)
    aL = np.abs(out.L)
    out.G = float((aL @ (np.abs(out.d) * (aL.T @ np.ones(n)))).max()) if out.bad < 0 else float("nan")
    out.norm = float(np.abs(full).sum(axis=1).max())
    return out


def coefficients(omega, dm, ds):
    """(alpha, beta) of S(omega) = alpha A + beta M as slod_lod_harmonic_response forms them: one rounding per part."""
    omega = np.asarray(omega, dtype=np.float64)
    return 1.0 + 1j * (omega * ds), -(omega * omega) + 1j * (omega * dm)


def combined(A, M, alpha, beta):
    """alpha A + beta M as the scatter kernel rounds it: re = (a_r A) + (b_r M), im = (a_i A) + (b_i M)."""
    alpha, beta = complex(alpha), complex(beta)
    return (alpha.real * A + beta.real * M) + 1j * (alpha.imag * A + beta.imag * M)


def system(A, M, omega, dm, ds):
    alpha, beta = coefficients(omega, dm, ds)
    return combined(A, M, alpha, beta)


def modal_response(lam, X, b, omega, dm, ds):
    """sum_j x_j (x_j^T b) / (lam_j (1 + i omega ds) + i omega dm - omega^2), (lam, X) of scipy's eigh(A, M) (X^T M X = I)."""
    den = lam * (1.0 + 1j * omega * ds) + 1j * omega * dm - omega * omega
    return X @ ((X.T @ b) / (den[:, None] if np.ndim(b) == 2 else den))


def polished_spectrum(A, M, X):
    """The Rayleigh quotients x_j^T A x_j / x_j^T M x_j of scipy's modes in np.longdouble, rounded to float64.  LAPACK's
    eigenvalues carry an absolute error of about u lam_n; exactly on a resonance of width 2 zeta lam_j the modal sum would
    inherit u lam_n / (2 zeta lam_j), 6e-10 at zeta = 0.05 % and lam_n / lam_1 = 5e3.  The quotient's error is quadratic in
    the mode's, so its relative error is the rounding to float64."""
    Xl = X.astype(np.longdouble)
    num = np.einsum("ij,ij->j", Xl, A.astype(np.longdouble) @ Xl)
    den = np.einsum("ij,ij->j", Xl, M.astype(np.longdouble) @ Xl)
    return np.array(num / den, dtype=np.float64)


def dampings(lam):
    """[(label, damp_mass, damp_stiff)]"""
    w1 = float(np.sqrt(lam[0]))
    dm, ds = 0.02 * w1, 1e-3 / w1
    return [("mass", dm, 0.0), ("stiff", 0.0, ds), ("both", dm, ds)]


def rule_frequencies(lam):
    n, w = len(lam), np.sqrt(lam)
    return [float(x) for x in (w[0], w[1], w[n // 4 - 1], w[n // 2 - 1], w[n - 1], 0.5 * w[0], 0.5 * (w[2] + w[3]), 2.0 * w[n - 1])]


def qualify(A, M, omega, dm, ds, perm=None):
    """The first of omega, omega (1 + 1/64), .. (eight moves at most) whose yardstick has no bad pivot and growth <= GROWTH_CAP:
    (omega, yardstick, moves).  None qualifies: AssertionError with what was seen."""
    perm = np.arange(A.shape[0]) if perm is None else perm
    seen = []
    for move in range(MOVES + 1):
        S = system(A, M, omega, dm, ds)[np.ix_(perm, perm)]
        ref = zldl_reference(S)
        growth = ref.G / ref.norm
        seen.append((omega, ref.bad, growth))
        if ref.bad < 0 and growth <= GROWTH_CAP:
            return omega, ref, move
        omega *= MOVE
    raise AssertionError("no frequency qualifies: %r" % seen)


def sweep(lam, A, M, perm=None, extra=0):
    """{damping label: (dm, ds, [(omega, yardstick, moves)])} at the eight frequencies of the rule and `extra` more, evenly
    spaced in [sqrt(lam_1) / 2, 2 sqrt(lam_n)], every one qualified."""
    w = rule_frequencies(lam)
    if extra:
        w += [float(x) for x in np.linspace(0.5 * np.sqrt(lam[0]), 2.0 * np.sqrt(lam[-1]), extra)]
    return {label: (dm, ds, [qualify(A, M, x, dm, ds, perm) for x in w]) for label, dm, ds in dampings(lam)}


def zeta(S, G, x, rhs):
    """Normwise backward error per column relative to G, the residual in extended precision."""
    r = rhs.astype(np.clongdouble) - S.astype(np.clongdouble) @ x.astype(np.clongdouble)
    return np.array(np.abs(r).max(axis=0) / (G * np.abs(x).max(axis=0) + np.abs(rhs).max(axis=0)), dtype=np.float64)


# ---- the four cases of the LDL^T tests with their spectrum, modes and qualified sweeps (needs a GPU)

_cases = {}


def harmonic_case(so, name):
    """ldl_case(name) with .X (modes, X^T M X = I) and .sweep (the rule at the three dampings); built once."""
    import scipy.linalg as sl
    if name not in _cases:
        c = ldl_case(so, name)
        c.X = sl.eigh(c.A, c.M)[1]
        c.lam_h = polished_spectrum(c.A, c.M, c.X)
        c.sweep = sweep(c.lam_h, c.A, c.M, c.perm)
        _cases[name] = c
    return _cases[name]
