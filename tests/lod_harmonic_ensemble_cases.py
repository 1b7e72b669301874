"""Helpers of the tests of the frequency response of a coefficient ensemble (slod_lod_factor_create_zldl_ensemble,
slod_lod_factor_solve_complex_ensemble, slod_lod_harmonic_response_ensemble); a plain module like lod_harmonic_cases.py,
whose yardstick, modal response, bars and single-member rule it shares.  Nothing in the rule, the column map or the model of
`quantities` calls the library, so test_lod_harmonic_ensemble_reference.py checks them on the CPU.

The layout, stated once: K members, F frequencies, n_rhs load columns.
  factor member     j = k K + m                    frequency k on the matrices of member m
  response column   (k K + m) n_rhs + c            of (d_u_re, d_u_im)
  load column       m n_rhs + c                    shared by all frequencies
  chunks            [64 i, min(64 (i + 1), F K))   of the flat j; a chunk may start and end inside a frequency

The ensemble sweep rule.  Frequencies: the eight of hc.rule_frequencies(lam of member 0), then sqrt(lam_1) of every other
member, so that each member meets its own first resonance.  Dampings: hc.dampings(lam of member 0).  A frequency qualifies
when the yardstick hc.zldl_reference of EVERY member has no bad pivot and growth <= GROWTH_CAP; otherwise it moves up by
1 + 1/64, at most 8 times, for all members together; none qualifies: AssertionError with the growths seen (never a skip).

quantities = (u^H M u, u^H A u, Re u^H b, Im u^H b) in np.longdouble is the model of the call's fourth output.  Its error
bar per column (nrow rows, cap s terms per row product, U = 2^-53):
  (nrow + cap s + 4) U sum_i |u_i| (|A| |u|)_i      for u^H A u (M alike),    ... sum_i |u_i| |b_i|   for the two parts of u^H b:
recursive summation over nrow rows on top of a cap s-term fma chain and the four roundings of the row's own products and sum.
"""
import numpy as np

import lod_cases                      # noqa: F401  (NAN, _bits, _torch for the GPU tests that import this module)
import lod_eig_direct_cases as ec     # ensemble_case, stack, dense
import lod_harmonic_cases as hc
from lod_eig_direct_cases import dense, ensemble_case, stack   # noqa: F401

CHUNK = 64
SURROGATE_CONTRASTS = (1.0, 1e2, 1e4)


# ---- the layout

def column(k, m, c, K, n_rhs):
    return (k * K + m) * n_rhs + c


def chunks(F, K):
    """[(j0, j1)] of the flat factor-member index."""
    return [(j0, min(j0 + CHUNK, F * K)) for j0 in range(0, F * K, CHUNK)]


def deinterleave(U, F, K, n_rhs):
    """The first F K n_rhs columns of a [rows][ld] array as [rows][F][K][n_rhs]."""
    U = np.asarray(U)
    return U[:, :F * K * n_rhs].reshape(U.shape[0], F, K, n_rhs)


# ---- the rule

def ensemble_frequencies(lams):
    return hc.rule_frequencies(lams[0]) + [float(np.sqrt(lam[0])) for lam in lams[1:]]


def qualify_joint(As, Ms, omega, dm, ds, perm=None):
    """The first of omega, omega (1 + 1/64), .. (eight moves at most) at which every member's yardstick has no bad pivot
    and growth <= GROWTH_CAP: (omega, [yardstick per member], moves)."""
    perm = np.arange(As[0].shape[0]) if perm is None else perm
    seen = []
    for move in range(hc.MOVES + 1):
        refs = [hc.zldl_reference(hc.system(A, M, omega, dm, ds)[np.ix_(perm, perm)]) for A, M in zip(As, Ms)]
        growths = [r.G / r.norm for r in refs]
        seen.append((omega, [r.bad for r in refs], growths))
        if all(r.bad < 0 for r in refs) and all(g <= hc.GROWTH_CAP for g in growths):
            return omega, refs, move
        omega *= hc.MOVE
    raise AssertionError("no frequency qualifies: %r" % seen)


def ensemble_sweep(lams, As, Ms, perm=None, extra=0):
    """{damping label: (dm, ds, [(omega, [yardstick per member], moves)])} at the frequencies of the rule and `extra` more,
    evenly spaced in [sqrt(lam_1) / 2, 2 sqrt(lam_n)] of member 0, every one qualified for all members."""
    w = ensemble_frequencies(lams)
    if extra:
        w += [float(x) for x in np.linspace(0.5 * np.sqrt(lams[0][0]), 2.0 * np.sqrt(lams[0][-1]), extra)]
    return {label: (dm, ds, [qualify_joint(As, Ms, x, dm, ds, perm) for x in w]) for label, dm, ds in hc.dampings(lams[0])}


# ---- the model of `quantities`

def quantities_model(A, M, u, b):
    """(u^H M u, u^H A u, Re u^H b, Im u^H b) per column of u in np.longdouble: [columns][4]."""
    ul, bl = u.astype(np.clongdouble), b.astype(np.clongdouble)
    out = np.zeros((u.shape[1], 4), dtype=np.longdouble)
    for q, S in enumerate((M, A)):
        Su = S.astype(np.longdouble) @ ul
        out[:, q] = (ul.real * Su.real + ul.imag * Su.imag).sum(axis=0)
    ub = (np.conj(ul) * bl).sum(axis=0)
    out[:, 2], out[:, 3] = ub.real, ub.imag
    return out


def quantities_bars(A, M, u, b, nrow, terms):
    """The error bar of every entry of quantities_model, [columns][4]."""
    au, ab = np.abs(u).astype(np.longdouble), np.abs(b).astype(np.longdouble)
    c = (nrow + terms + 4) * hc.U
    qa = (au * (np.abs(A).astype(np.longdouble) @ au)).sum(axis=0)
    qm = (au * (np.abs(M).astype(np.longdouble) @ au)).sum(axis=0)
    qb = (au * ab).sum(axis=0)
    return np.array(c * np.stack([qm, qa, qb, qb], axis=1), dtype=np.float64)


# ---- the surrogate ensembles of the CPU check: Q1 pencils of contrast 1, 1e2, 1e4 on one grid

def surrogate_ensemble(inner):
    """([A_m], [M_m], [lam_m], [X_m]) with polished spectra."""
    import scipy.linalg as sl
    As, Ms, lams, Xs = [], [], [], []
    for contrast in SURROGATE_CONTRASTS:
        A, M = hc.q1_pencil(inner, contrast)
        X = sl.eigh(A, M)[1]
        As.append(A), Ms.append(M), Xs.append(X), lams.append(hc.polished_spectrum(A, M, X))
    return As, Ms, lams, Xs


# ---- the three ensemble cases with spectra, modes, factor order and the qualified sweep (needs a GPU)

_cases = {}


def harmonic_ensemble_case(so, name):
    """ec.ensemble_case(name) with per member .lam_h, .X, and .perm, .hbw, .sweep (the ensemble rule); built once."""
    import scipy.linalg as sl
    from lod_ldl_cases import factor_order
    if name not in _cases:
        c = ensemble_case(so, name)
        c.X = [sl.eigh(A, M)[1] for A, M in zip(c.A, c.M)]
        c.lam_h = [hc.polished_spectrum(A, M, X) for A, M, X in zip(c.A, c.M, c.X)]
        c.perm = factor_order(c)
        w = 2 * c.g.cfg.oversampling + 1
        c.hbw = c.s * (w * c.g.N + w) + c.s - 1
        c.sweep = ensemble_sweep(c.lam_h, c.A, c.M, c.perm)
        _cases[name] = c
    return _cases[name]
