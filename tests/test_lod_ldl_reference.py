"""The measuring stick of the LDL^T tests, checked on the CPU (as test_lod_slab_reference.py checks the slabs): the
unpivoted LDL^T in numpy of lod_ldl_cases.py and its shift rule, on the surrogate pencil of the feasibility check -- Q1
stiffness and mass on 8^2 and 16^2 interior nodes (64 and 256 unknowns), a random coefficient of contrast 1e4, fixed seed.
At the five shifts of the GPU tests (the rule at t = 1, rows / 4, rows / 2; lambda_1 / 2; 2 lambda_max):
  - the yardstick's inertia equals the number of eigenvalues of scipy's eigh(A, M) below sigma;
  - the growth G / ||S||_inf is at most 1e4 at every shift the rule chose;
  - L D L^T reproduces S, and a solve with the yardstick's factor meets the backward bound of the GPU tests,
    eta <= (3 (b + 1) + 1) (b + 1) 2^-53 relative to G, b = the half bandwidth of the row-major grid.
Nothing here calls the library."""
import numpy as np
import pytest

import lod_ldl_cases as lc


@pytest.mark.parametrize("inner", [8, 16])
def test_ldl_yardstick_on_the_q1_surrogate(inner):
    import scipy.linalg as sl
    A, M = lc.q1_pencil(inner)
    rows, b = inner * inner, inner + 1
    assert A.shape == (rows, rows) and np.array_equal(A, A.T) and np.array_equal(M, M.T)
    lam = sl.eigh(A, M, eigvals_only=True)
    assert lam[0] > 0.0
    rng = np.random.default_rng(211)
    shifts = lc.five_shifts(lam, A, M)
    assert [g for _, _, g, _ in shifts[3:]] == [0, rows]
    for k, (label, sigma, below, ref) in enumerate(shifts):
        S = A - sigma * M
        assert ref.bad < 0
        assert below == int((lam < sigma).sum())
        assert (ref.n_negative, ref.n_positive) == (below, rows - below), (label, ref.n_negative, below)
        growth = ref.G / ref.norm
        assert ref.norm == np.abs(S).sum(axis=1).max()
        if k < 3:
            assert growth <= lc.GROWTH_CAP, (label, growth)
        # the factor outside the band is exactly zero: no fill beyond the half bandwidth
        assert not np.tril(ref.L, -(b + 1)).any()
        recon = (ref.L * ref.d) @ ref.L.T
        assert np.abs(recon - S).max() <= lc.bound(b) * ref.G, (label, np.abs(recon - S).max())
        worst = 0.0
        for n in (1, 3, 17):
            rhs = rng.uniform(-1.0, 1.0, (rows, n))
            x = lc.banded_solve(ref, rhs)
            e = lc.eta(S, ref.G, x, rhs)
            worst = max(worst, e.max())
            assert (e <= lc.bound(b)).all(), (label, n, e.max(), lc.bound(b))
        print("q1 %d^2 %s: sigma %.6e, %d below, growth %.3e, backward error %.3e (bound %.3e)"
              % (inner, label, sigma, below, growth, worst, lc.bound(b)))


def test_ldl_yardstick_reports_the_first_bad_pivot():
    A, M = lc.q1_pencil(4)
    S = A.copy()
    S[0, 0] = 0.0
    assert lc.ldl_reference(S).bad == 0
    S = A.copy()
    S[9, 5] = float("nan")                 # lower triangle: row 9 is the first whose pivot sees it
    S[2, 7] = float("nan")                 # upper triangle: never read
    assert lc.ldl_reference(S).bad == 9


def test_shift_rule_fails_when_no_gap_qualifies():
    """Eight gaps of a spectrum with a multiple eigenvalue: no midpoint has a relative gap of 1e-6, and the rule raises."""
    lam = np.ones(12)
    with pytest.raises(AssertionError):
        lc.shift_at(lam, np.eye(12), np.eye(12), 1)
