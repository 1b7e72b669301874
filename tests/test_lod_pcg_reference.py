"""The yardstick of the preconditioned-CG tests, checked on the CPU (as test_lod_ldl_reference.py checks the LDL^T one):
pcg_reference of lod_pcg_cases.py on the library-free SPD pencil lod_ldl_cases.q1_pencil (Q1 stiffness on 8^2 interior
nodes, a random coefficient of contrast 1e4, fixed seed).
  - With P = A the reference stops at count 1 for tol = 1e-10.
  - With A' = A + sum_{i<r} a_ii e_i e_i^T, r = 1, 3, 8, and P = A, P^-1 A' is the identity plus a matrix of rank r, so CG
    ends after at most r + 1 iterations: asserted of the reference.
  - The reference's solution equals numpy.linalg.solve to 1e-12 relative.  That is asked of the run at tol = 1e-13: a stop
    at 1e-10 promises the solution only to 1e-10 times the condition number (r = 8 stops an iteration early there, at
    7e-12), and the count at 1e-13 still meets r + 1.
Nothing here calls the library."""
import numpy as np
import pytest

import lod_ldl_cases as lc
import lod_pcg_cases as pc

TOL = 1e-10


def _pencil():
    A, M = lc.q1_pencil(8)
    b = np.random.default_rng(311).uniform(-1.0, 1.0, A.shape[0])
    return A, M, b


def _close(u, A, b):
    x = np.linalg.solve(A, b)
    return np.linalg.norm(u - x) / np.linalg.norm(x)


def test_factor_of_the_matrix_itself_stops_after_one_iteration():
    A, M, b = _pencil()
    for S in (A, M, M + 0.01 * A):
        u, count, hist = pc.pcg_reference(S, pc.dense_solver(S), b, TOL, 50)
        assert count == 1 and len(hist) == 2 and hist[0] == 1.0 and hist[1] <= TOL
        assert _close(u, S, b) <= 1e-12
        lo, hi, res = pc.bracket(S, pc.dense_solver(S), b, TOL)
        assert (lo, hi) == (1, 1) and res <= TOL
        pc.check_bracket("self", 1, lo, hi)


@pytest.mark.parametrize("r", [1, 3, 8])
def test_rank_r_perturbation_ends_in_r_plus_one_iterations(r):
    A, M, b = _pencil()
    rows = np.arange(r)
    A2 = pc.doubled_diagonal(A, rows)
    assert np.linalg.matrix_rank(A2 - A) == r
    u, count, hist = pc.pcg_reference(A2, pc.dense_solver(A), b, TOL, 50)
    assert 1 <= count <= r + 1, (r, count, hist)
    u, tight, _ = pc.pcg_reference(A2, pc.dense_solver(A), b, 1e-13, 50)
    assert count <= tight <= r + 1
    assert _close(u, A2, b) <= 1e-12
    _, jac, _ = pc.jacobi_reference(A2, b, TOL, 5000)
    print("r = %d: %d iterations with the factor of A, %d with Jacobi, residuals %s" % (r, count, jac, ["%.1e" % h for h in hist]))
    assert jac > r + 2


def test_stop_rule_edges():
    A, M, b = _pencil()
    u, count, hist = pc.pcg_reference(A, pc.dense_solver(A), np.zeros_like(b), TOL, 50)
    assert count == 0 and not u.any() and hist == [0.0]
    u, count, hist = pc.pcg_reference(A, pc.dense_solver(M), b, TOL, 0)
    assert count == 0 and not u.any() and hist == [1.0]
    u, count, hist = pc.pcg_reference(A, pc.dense_solver(M), b, TOL, 1)
    assert count == 1 and len(hist) == 2
    u, count, _ = pc.jacobi_reference(A, b, TOL, 5000)
    assert 1 < count < 5000 and _close(u, A, b) <= 1e-8
    with pytest.raises(AssertionError):
        pc.check_bracket("wide", 5, 1, 9)
    with pytest.raises(AssertionError):
        pc.check_bracket("outside", 4, 1, 3)


def test_few_mode_load_ends_a_far_preconditioner_in_m_iterations():
    A, M, b = _pencil()
    P = M + 1e-3 * A                                                         # far from A
    _, general, _ = pc.pcg_reference(A, pc.dense_solver(P), b, TOL, 500)
    for m in (3, 5):
        f = pc.few_mode_load(A, P, m)
        u, count, hist = pc.pcg_reference(A, pc.dense_solver(P), f, TOL, 500)
        lo, hi, _ = pc.bracket(A, pc.dense_solver(P), f, TOL)
        assert count == m < general and hi - lo <= pc.BRACKET_CAP and lo <= count <= hi, (m, count, general, lo, hi, hist)
        assert _close(u, A, f) <= 1e-8
