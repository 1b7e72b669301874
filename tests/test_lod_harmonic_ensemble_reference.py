"""The measuring sticks of the ensemble frequency-response tests, checked on the CPU: the ensemble sweep rule, the column
map and the model of `quantities` of lod_harmonic_ensemble_cases.py, on surrogate ensembles -- Q1 stiffness and mass on
5^2 and 8^2 interior nodes (25 and 64 rows), members of contrast 1, 1e2 and 1e4.
  - the rule gives ten frequencies that qualify jointly at the three dampings (and need no move here);
  - the yardstick's solve of every (frequency, member) agrees with the modal response to FORWARD;
  - the model of quantities satisfies  omega (dm u^H M u + ds u^H A u) = Im u^H b  and
    u^H A u - omega^2 u^H M u = Re u^H b  (the two parts of u^H S u = u^H b) to 1e-10 of the sum of the moduli of the
    identity's terms;
  - the column map (k K + m) n_rhs + c and the flat chunk boundaries are what the header states.
Nothing here calls the library."""
import numpy as np
import pytest

import lod_harmonic_cases as hc
import lod_harmonic_ensemble_cases as he
from lod_ldl_cases import banded_solve


@pytest.fixture(scope="module", params=[5, 8], ids=lambda p: "q1_%d" % p)
def ensemble(request):
    inner = request.param
    As, Ms, lams, Xs = he.surrogate_ensemble(inner)
    assert As[0].shape == (inner * inner,) * 2 and all(lam[0] > 0.0 for lam in lams)
    return inner, As, Ms, lams, Xs, he.ensemble_sweep(lams, As, Ms)


def test_rule_qualifies_jointly(ensemble):
    inner, As, Ms, lams, Xs, sweeps = ensemble
    first = he.ensemble_frequencies(lams)
    assert len(first) == 10 and first[:8] == hc.rule_frequencies(lams[0])
    assert first[8:] == [float(np.sqrt(lams[1][0])), float(np.sqrt(lams[2][0]))]
    assert [label for label in sweeps] == [label for label, _, _ in hc.dampings(lams[0])]
    worst = 0.0
    for label, (dm, ds, freqs) in sweeps.items():
        assert len(freqs) == 10
        for (omega, refs, moves), w in zip(freqs, first):
            assert len(refs) == 3 and all(r.bad < 0 for r in refs)
            growth = max(r.G / r.norm for r in refs)
            worst = max(worst, growth)
            assert growth <= hc.GROWTH_CAP, (label, omega, growth)
            assert moves == 0 and omega == w, (label, omega, moves)            # the surrogates need no move
    print("q1 %d^2 ensemble: worst growth %.3e" % (inner, worst))


def test_rule_moves_all_members_together_and_fails_loudly():
    A, M = hc.q1_pencil(4)
    bad = np.ones_like(A)
    bad[0, 0] = 0.0
    with pytest.raises(AssertionError) as e:                                   # one member never qualifies: nobody does
        he.qualify_joint([A, bad], [M, np.zeros_like(M)], 1.0, 0.1, 0.0)
    assert "no frequency qualifies" in str(e.value) and str(e.value).count("(") >= hc.MOVES + 1
    omega, refs, moves = he.qualify_joint([A, A], [M, M], 3.0, 0.1, 0.0)
    assert (omega, moves, len(refs)) == (3.0, 0, 2)


def test_yardstick_solve_agrees_with_the_modal_response(ensemble):
    inner, As, Ms, lams, Xs, sweeps = ensemble
    rows = inner * inner
    rng = np.random.default_rng(601)
    load = rng.uniform(-1.0, 1.0, (rows, 3)) + 1j * rng.uniform(-1.0, 1.0, (rows, 3))
    load[:, 0] = load[:, 0].real
    worst = 0.0
    for label, (dm, ds, freqs) in sweeps.items():
        for omega, refs, _ in freqs:
            for m, ref in enumerate(refs):
                x = banded_solve(ref, load)
                modal = hc.modal_response(lams[m], Xs[m], load, omega, dm, ds)
                err = (np.abs(x - modal).max(axis=0) / np.abs(x).max(axis=0)).max()
                worst = max(worst, err)
                assert err <= hc.FORWARD, (label, omega, m, err)
    print("q1 %d^2 ensemble: yardstick solve against the modal response %.3e" % (inner, worst))


def test_quantities_model_satisfies_both_parts_of_the_energy_identity(ensemble):
    inner, As, Ms, lams, Xs, sweeps = ensemble
    rows = inner * inner
    rng = np.random.default_rng(603)
    load = rng.uniform(-1.0, 1.0, (rows, 3)) + 1j * rng.uniform(-1.0, 1.0, (rows, 3))
    load[:, 0] = load[:, 0].real
    worst = 0.0
    for label, (dm, ds, freqs) in sweeps.items():
        for omega, refs, _ in freqs:
            for m, ref in enumerate(refs):
                u = banded_solve(ref, load)
                q = np.array(he.quantities_model(As[m], Ms[m], u, load), dtype=np.float64)
                uMu, uAu, re, im = q.T
                assert (uMu > 0.0).all() and (uAu > 0.0).all()
                for off, scale in ((omega * (dm * uMu + ds * uAu) - im, omega * (dm * uMu + ds * uAu) + np.abs(im)),
                                   (uAu - omega * omega * uMu - re, uAu + omega * omega * uMu + np.abs(re))):
                    worst = max(worst, (np.abs(off) / scale).max())
                    assert (np.abs(off) <= 1e-10 * scale).all(), (label, omega, m, off, scale)
                bars = he.quantities_bars(As[m], Ms[m], u, load, rows, 9)
                assert bars.shape == (3, 4) and (bars > 0.0).all() and (bars[:, 2] == bars[:, 3]).all()
    zero = he.quantities_model(As[0], Ms[0], np.zeros((rows, 1), dtype=complex), np.zeros((rows, 1), dtype=complex))
    assert not zero.any()
    print("q1 %d^2 ensemble: energy identities off by %.3e of their terms" % (inner, worst))


def test_column_map_and_chunk_boundaries():
    F, K, n = 23, 3, 3
    cols = [he.column(k, m, c, K, n) for k in range(F) for m in range(K) for c in range(n)]
    assert cols == list(range(F * K * n))                                      # frequency-major, member-minor, a bijection
    assert he.column(21, 1, 0, K, 1) == 64                                     # the boundary at j = 64 is inside frequency 21
    assert he.chunks(F, K) == [(0, 64), (64, 69)]
    assert he.chunks(2, 65) == [(0, 64), (64, 128), (128, 130)]
    assert he.chunks(1, 1) == [(0, 1)] and he.chunks(1, 64) == [(0, 64)]
    U = np.arange(2 * (F * K * n + 4), dtype=np.float64).reshape(2, -1)        # two rows, four padding columns
    D = he.deinterleave(U, F, K, n)
    assert D.shape == (2, F, K, n)
    for k, m, c in ((0, 0, 0), (5, 2, 1), (22, 2, 2)):
        assert D[1, k, m, c] == U[1, he.column(k, m, c, K, n)]
    # with n_rhs = 1 a frequency's block is an ensemble multi-vector, column = member, at offset k K
    assert [he.column(7, m, 0, K, 1) for m in range(K)] == [7 * K + m for m in range(K)]
