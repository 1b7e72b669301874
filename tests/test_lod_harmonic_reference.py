"""The measuring sticks of the frequency-response tests, checked on the CPU (as test_lod_ldl_reference.py checks the real
yardstick): the unpivoted complex LDL^T in numpy, the modal response and the sweep rule of lod_harmonic_cases.py, on the
surrogate pencil of the feasibility check -- Q1 stiffness and mass on 8^2 and 16^2 interior nodes, contrast 1 and 1e4.
  - L D L^T reproduces S to bound(b) G, b = the half bandwidth of the row-major grid;
  - every frequency of the rule, at the three dampings, stays under the growth cap (and needs no move here);
  - the modal response equals numpy.linalg.solve(S, b) to 1e-10 of max |u|;
  - with alpha, beta real the yardstick's imaginary parts are exactly zero and L, d equal ldl_reference's to 1e-13;
  - the power identity  omega u^H C u = Im(u^H b)  holds for the dense solution to 1e-10 of |u^H b|.
Nothing here calls the library."""
import numpy as np
import pytest

import lod_harmonic_cases as hc


@pytest.fixture(scope="module", params=[(8, 1.0), (8, 1e4), (16, 1.0), (16, 1e4)], ids=lambda p: "q1_%d_contrast_%g" % p)
def pencil(request):
    import scipy.linalg as sl
    inner, contrast = request.param
    A, M = hc.q1_pencil(inner, contrast)
    lam, X = sl.eigh(A, M)
    assert np.abs(hc.polished_spectrum(A, M, X) - lam).max() <= 64 * hc.U * lam[-1]      # LAPACK's absolute error
    lam = hc.polished_spectrum(A, M, X)
    assert lam[0] > 0.0 and np.array_equal(A, A.T) and np.array_equal(M, M.T)
    return inner, A, M, lam, X, hc.sweep(lam, A, M)


def test_rule_gives_eight_frequencies_under_the_cap(pencil):
    inner, A, M, lam, X, sweeps = pencil
    assert len(hc.rule_frequencies(lam)) == 8 and len(sweeps) == 3
    worst = 0.0
    for label, (dm, ds, freqs) in sweeps.items():
        assert len(freqs) == 8
        for (omega, ref, moves), first in zip(freqs, hc.rule_frequencies(lam)):
            growth = ref.G / ref.norm
            worst = max(worst, growth)
            assert ref.bad < 0 and growth <= hc.GROWTH_CAP, (label, omega, growth)
            assert moves == 0 and omega == first, (label, omega, moves)       # the surrogate needs no move
    print("q1 %d^2: worst growth %.3e" % (inner, worst))


def test_yardstick_reproduces_the_matrix(pencil):
    inner, A, M, lam, X, sweeps = pencil
    b = inner + 1
    for label, (dm, ds, freqs) in sweeps.items():
        for omega, ref, _ in freqs:
            S = hc.system(A, M, omega, dm, ds)
            assert ref.norm == np.abs(S).sum(axis=1).max()
            assert not np.tril(ref.L, -(b + 1)).any()                          # no fill beyond the half bandwidth
            recon = (ref.L * ref.d) @ ref.L.T
            assert np.abs(recon - S).max() <= hc.bound(b) * ref.G, (label, omega, np.abs(recon - S).max())


def test_modal_response_and_power_identity(pencil):
    inner, A, M, lam, X, sweeps = pencil
    rows = inner * inner
    rng = np.random.default_rng(401)
    load = rng.uniform(-1.0, 1.0, (rows, 3)) + 1j * rng.uniform(-1.0, 1.0, (rows, 3))
    load[:, 0] = load[:, 0].real
    worst = 0.0
    for label, (dm, ds, freqs) in sweeps.items():
        Cd = dm * M + ds * A
        for omega, ref, _ in freqs:
            S = hc.system(A, M, omega, dm, ds)
            u = np.linalg.solve(S, load)
            modal = hc.modal_response(lam, X, load, omega, dm, ds)
            err = np.abs(modal - u).max() / np.abs(u).max()
            worst = max(worst, err)
            assert err <= 1e-10, (label, omega, err)
            for c in range(3):
                ub = np.vdot(u[:, c], load[:, c])                              # u^H b
                power = omega * np.vdot(u[:, c], Cd @ u[:, c])
                assert abs(power.imag) <= 1e-10 * abs(ub)
                assert abs(power.real - ub.imag) <= 1e-10 * abs(ub), (label, omega, c, power.real, ub.imag)
    print("q1 %d^2: modal response against the dense solve %.3e" % (inner, worst))


def test_real_coefficients_give_the_real_yardstick(pencil):
    inner, A, M, lam, X, sweeps = pencil
    for sigma in (0.0, 0.5 * lam[0], 2.0 * lam[-1]):
        S = hc.combined(A, M, 1.0, -sigma)
        assert not S.imag.any() and np.array_equal(S.real, 1.0 * A + (-sigma) * M)
        z, r = hc.zldl_reference(S), hc.ldl_reference(S.real)
        assert z.bad < 0 and r.bad < 0
        assert not z.L.imag.any() and not z.d.imag.any()
        assert np.abs(z.L.real - r.L).max() <= 1e-13 * np.abs(r.L).max()
        assert (np.abs(z.d.real - r.d) <= 1e-13 * np.abs(r.d)).all()
        assert z.norm == r.norm and abs(z.G - r.G) <= 1e-12 * r.G


def test_yardstick_reports_the_first_bad_pivot():
    A, M = hc.q1_pencil(4)
    S = hc.system(A, M, 3.0, 0.1, 0.0)
    Z = S.copy()
    Z[0, 0] = 0.0
    assert hc.zldl_reference(Z).bad == 0
    Z = S.copy()
    Z[9, 5] = complex(0.0, float("nan"))    # lower triangle: row 9 is the first whose pivot sees it
    Z[2, 7] = float("nan")                  # upper triangle: never read
    assert hc.zldl_reference(Z).bad == 9
    assert hc.zldl_reference(np.zeros((4, 4))).bad == 0


def test_rule_fails_when_no_frequency_qualifies():
    """A zero first pivot at every move: the rule raises with what it saw."""
    A = np.ones((6, 6))
    A[0, 0] = 0.0
    with pytest.raises(AssertionError) as e:
        hc.qualify(A, np.zeros((6, 6)), 1.0, 0.1, 0.0)
    assert "no frequency qualifies" in str(e.value)
