"""CPU tests of the multigrid reference of tests/mg_cases.py alone (no GPU, no library): the preconditioner it
describes is symmetric positive definite under the damping rule, the constant damping it replaces is not, the
reference in float64 stays within a few ulp of the one in longdouble, every stand-in mistake the GPU tests claim to
catch moves the compared quantity far beyond their bar, and the loads and tolerances of the iteration-count test
leave a factor 10 on either side of every burst end."""
import numpy as np
import pytest

import mg_cases as mg

SMALL = [c for c in mg.CASES if c[1] <= 8]      # the cases the mutants run on
ids = mg.case_id


def _eig_sym(B):
    return np.linalg.eigvalsh(0.5 * (B + B.T))


def test_level_rule():
    assert [mg.level_sizes(n) for n in (4, 6, 8, 10, 12, 16, 24, 64)] == \
        [[4, 2], [6, 3], [8, 4, 2], [10, 5], [12, 6, 3], [16, 8, 4, 2], [24, 12, 6, 3], [64, 32, 16, 8, 4, 2]]


def test_interpolation_has_no_weight_between_rim_and_interior():
    """Two mistakes cannot be seen by any test, by geometry: a restriction that also gathers the constrained fine
    nodes, and a prolongation that also writes them.  Both use the weights that tie a rim fine node to an interior
    coarse node, and the hat of an interior coarse node X covers the fine nodes 2X - 1 .. 2X + 1, all interior:
    those weights are exactly 0.  (The weights between a rim coarse node and interior fine nodes are not 0, but rim
    coarse values are 0 on every level.)"""
    for Nf in (4, 6, 8, 10, 12, 16):
        P = mg.p1d_all_nodes(Nf)
        assert np.all(P[[0, Nf], 1:Nf // 2] == 0.0)
        assert np.array_equal(P[1:Nf, 1:Nf // 2], mg._p1d(Nf, np.float64))


@pytest.mark.parametrize("case", mg.CASES, ids=ids)
def test_reference_is_symmetric_positive_definite(so, case):
    """B symmetric to rounding (the pre- and post-smoothing are transposes of each other in exact arithmetic; 1e-15 of
    max |B| is about 4 ulp), positive definite, and the spectrum of B A in (0, 1]: with omega_l lambda_max <= 1.6
    every smoother and the exact coarsest solve contract in the energy norm, so I - B A has its spectrum in [0, 1)."""
    A, _ = mg.problem(so, case)
    H = mg.hierarchy(so, case)
    B = mg.b_matrix(so, case)
    lmax = H.lambda_max()
    print("%s: levels %s, lambda_max(D^-1 A) %s, omega %s" % (ids(case), [L["N"] for L in H.lev], ["%.3f" % x for x in lmax],
                                                           ["%.3f" % float(L["omega"]) for L in H.lev]))
    for L, lm in zip(H.lev, lmax):
        if L["N"] > 2:
            assert float(L["omega"]) * lm <= mg.OMEGA_TARGET * (1 + 1e-12), (L["N"], lm)
            assert lm <= float(L["norm_inf"]) * (1 + 1e-12)
    assert np.abs(B - B.T).max() <= 1e-15 * np.abs(B).max()
    assert _eig_sym(B).min() > 0.0
    ev = np.linalg.eigvals(B @ A.toarray())
    assert np.abs(ev.imag).max() <= 1e-10
    print("    eig(B A) in [%.4g, %.12g], kappa %.1f" % (ev.real.min(), ev.real.max(), ev.real.max() / ev.real.min()))
    assert ev.real.min() > 0.0 and ev.real.max() <= 1.0 + 1e-12


@pytest.mark.parametrize("case", mg.CASES, ids=ids)
def test_constant_damping(so, case):
    """omega = 0.8 on every level, the damping before the rule: B is indefinite exactly where 0.8 lambda_max > 2 on
    some level, which are the elasticity cases at contrast 1e4 from NE = 8 on."""
    H = mg.hierarchy(so, case, omega=0.8)
    B = mg.b_matrix(so, case, omega=0.8)
    lmax = H.lambda_max()
    lo = _eig_sym(B).min()
    print("%s: omega 0.8, lambda_max per level %s, min eig(B) %.2e" % (ids(case), ["%.3f" % x for x in lmax], lo))
    if case in mg.INDEFINITE_TODAY:
        assert 0.8 * max(lmax) > 2.0 and lo < 0.0
    else:
        assert lo > 0.0


@pytest.mark.parametrize("case", [c for c in mg.CASES if c[1] <= mg.LONGDOUBLE_MAX_NE], ids=ids)
def test_float64_reference_against_longdouble(so, case):
    """e64 of u_1 and of the trajectory: a few ulp (at most 1e-14), so the floor 1e-13 decides most bars."""
    r = mg.reference_u1(so, case)
    _, et = mg.reference_trajectory(so, case)
    worst = max(float(r["e64_unit"].max()), float(r["e64_dense"].max()))
    print("%s: e64 u_1 unit %.1e, dense %.1e; trajectory %s" % (ids(case), r["e64_unit"].max(), r["e64_dense"].max(),
                                                               {k: "%.1e" % v for k, v in et.items()}))
    assert worst <= 1e-14 and max(et.values()) <= 1e-14


@pytest.mark.parametrize("mutant", mg.MUTANTS)
def test_mutant_moves_u1_beyond_the_bar(so, mutant):
    """Each stand-in mistake moves u_1 of some unit or dense load by at least 100 bars on at least one small case."""
    best = 0.0
    for case in SMALL:
        if mutant in ("galerkin_ab_swapped", "point_jacobi") and case[2] == 1:
            continue
        if mutant == "omega_on_N2" and mg.level_sizes(case[1])[-1] != 2:
            continue
        A, _ = mg.problem(so, case)
        ref, Bm = mg.reference_u1(so, case), mg.b_matrix(so, case, mutant=mutant)
        dofs, F = mg.unit_load_dofs(so, case), mg.dense_loads(so, case)
        moved = np.concatenate([mg.rel_dist(mg.first_step_unit(A, Bm)[:, dofs], ref["unit"]) / mg.bar(ref["e64_unit"]),
                                mg.rel_dist(mg.first_step(A, Bm, F), ref["dense"]) / mg.bar(ref["e64_dense"])])
        print("%s on %s: u_1 moves by %.1e bars at most, %.1e at least" % (mutant, ids(case), moved.max(), moved.min()))
        best = max(best, float(moved.max()))
    assert best >= 100.0


@pytest.mark.parametrize("case", mg.CASES, ids=ids)
def test_count_tolerance_keeps_clear_of_every_burst_end(so, case):
    f, tol, expected, ends = mg.count_case(so, case)
    print("%s: tol %s, expected %s iterations, residual at the burst ends %s" % (ids(case), tol, expected, ["%.1e" % e for e in ends]))
    assert tol is not None and expected >= mg.BURST
    assert not ((ends >= tol / 10) & (ends <= 10 * tol)).any()
    assert ends[expected // mg.BURST - 1] < tol and (ends[:expected // mg.BURST - 1] > tol).all()


def test_predicted_counts_on_the_65_grid(so):
    """Elasticity, contrast 1e4, 65^2 nodes: the reference with the rule, with the constant damping, and Jacobi."""
    it_mg, it_j = mg.predict_65(so)
    it_08, _ = mg.predict_65(so, omega=0.8)
    print("65^2 elasticity D1e4, reference: multigrid-CG %d (omega 0.8: %d), Jacobi-CG %d iterations" % (it_mg, it_08, it_j))
    assert dict(mg=it_mg, jacobi=it_j) == mg.PREDICTED_65
    assert it_08 > it_j
