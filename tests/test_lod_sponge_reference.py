"""CPU checks of the yardsticks of lod_sponge_cases.py on the Q1 surrogate pencil with 7^2 and 12^2 interior nodes: the
damped one-solve IRK form against the damped stage system, the energy identity of the damped trapezoidal rule, the
qualification of the rule frequencies with the sponge, the five-quantity model against u^H S u = u^H b, and the sponge
matrix itself.  Nothing here calls the library: the tests guard the references the GPU tests use.
"""
import numpy as np
import pytest

import lod_sponge_cases as sc

INNER = (7, 12)


@pytest.mark.parametrize("inner", INNER)
def test_one_solve_form_equals_the_stage_system(inner):
    A, M, D, lam = sc.q1_sponge_case(inner)
    n = A.shape[0]
    rng = np.random.default_rng(901)
    u0, v0 = rng.uniform(-1.0, 1.0, (n, 2)), np.sqrt(lam[n // 2]) * rng.uniform(-1.0, 1.0, (n, 2))
    loads = np.array([A @ rng.uniform(-1.0, 1.0, (n, 2)) for _ in range(6)])
    worst = 0.0
    for label, scheme in sc.SCHEMES:
        for dt in sc.wave_dts(lam):
            for dlabel, dm, ds in sc.sponge_dampings(lam):
                ru, rv = sc.wave_stage(A, M, D, scheme, dt, 3, u0, v0, dm, ds, loads)
                gu, gv = sc.wave_one_solve(A, M, D, scheme, dt, 3, u0, v0, dm, ds, loads)
                e = max(np.abs(gu - ru).max() / np.abs(ru).max(), np.abs(gv - rv).max() / np.abs(rv).max())
                worst = max(worst, e)
                assert e <= 1e-10, (inner, label, dt, dlabel, e)
    print("%d^2 nodes: one-solve form against the stage system %.3e" % (inner, worst))


@pytest.mark.parametrize("inner", INNER)
def test_trapezoidal_rule_obeys_the_energy_identity(inner):
    A, M, D, lam = sc.q1_sponge_case(inner)
    n = A.shape[0]
    rng = np.random.default_rng(902)
    u0, v0 = rng.uniform(-1.0, 1.0, (n, 3)), np.sqrt(lam[0]) * rng.uniform(-1.0, 1.0, (n, 3))
    dt, steps = 0.7 / np.sqrt(lam[0]), 10
    zero = np.zeros((n, 3))
    worst = 0.0
    for dlabel, dm, ds in sc.sponge_dampings(lam):
        Cd = dm * M + ds * A + D
        a0 = sc.newmark_accel(A, M, D, u0, v0, zero, dm, ds)
        us, vs, _ = sc.newmark(A, M, D, dt, 0.25, 0.5, steps, u0, v0, a0, lambda k: zero, dm, ds)
        kin, pot = sc.energies(A, M, us, vs)
        E = kin + pot
        vbar = 0.5 * (vs[1:] + vs[:-1])
        loss = dt * np.einsum("kic,ij,kjc->kc", vbar, Cd, vbar)
        e = float((np.abs((E[1:] - E[:-1]) + loss) / E[0]).max())
        worst = max(worst, e)
        assert e <= 1e-12, (inner, dlabel, e)
        assert (E[1:] <= E[:-1] + 1e-12 * E[0]).all() and (E[-1] < E[0]).all()
    print("%d^2 nodes: trapezoidal energy identity off by %.3e of E_0" % (inner, worst))


@pytest.mark.parametrize("inner", (4, 8, 12, 16))
def test_rule_frequencies_qualify_without_a_move(inner):
    A, M, D, lam = sc.q1_sponge_case(inner)
    worst = 0.0
    for label, (dm, ds, freqs) in sc.sweep(lam, A, M, D).items():
        for w, ref, moves in freqs:
            assert moves == 0, (inner, label, w, moves)
            worst = max(worst, ref.G / ref.norm)
    step = 0.0
    for _, scheme in sc.SCHEMES:
        for dt in sc.wave_dts(lam):
            for _, dm, ds in sc.sponge_dampings(lam):
                g, ref = sc.growth_of(sc.irk_system(A, M, D, scheme, dt, dm, ds))
                assert ref.bad < 0 and g <= sc.GROWTH_CAP
                step = max(step, g)
    print("%d^2 nodes: worst growth of the sweep %.3f, of the IRK step matrices %.3f" % (inner, worst, step))


@pytest.mark.parametrize("inner", INNER)
def test_quantities_balance(inner):
    A, M, D, lam = sc.q1_sponge_case(inner)
    n = A.shape[0]
    rng = np.random.default_rng(903)
    b = rng.uniform(-1.0, 1.0, (n, 3)) + 1j * rng.uniform(-1.0, 1.0, (n, 3))
    worst = 0.0
    for label, (dm, ds, freqs) in sc.sweep(lam, A, M, D).items():
        for w, _, _ in freqs:
            u = np.linalg.solve(sc.harmonic_system(A, M, D, w, dm, ds), b)
            q, mag = sc.quantities(A, M, D, u, b)
            re = q[:, 1] - w * w * q[:, 0] - q[:, 3]
            im = w * (dm * q[:, 0] + ds * q[:, 1] + q[:, 2]) - q[:, 4]
            s_re = mag[:, 1] + w * w * mag[:, 0] + mag[:, 3]
            s_im = w * (dm * mag[:, 0] + ds * mag[:, 1] + mag[:, 2]) + mag[:, 4]
            e = float(max((np.abs(re) / s_re).max(), (np.abs(im) / s_im).max()))
            worst = max(worst, e)
            assert e <= 1e-10, (inner, label, w, e)
    print("%d^2 nodes: the two parts of u^H S u = u^H b off by %.3e of the sum of the moduli" % (inner, worst))


def test_sponge_matrix_is_semi_definite_and_rank_deficient():
    A, M, D, lam = sc.q1_sponge_case(12)
    assert np.array_equal(D, D.T)
    ev = np.linalg.eigvalsh(D)
    assert ev[0] >= -1e-12 * ev[-1] and ev[-1] > 0.0
    zero = ~D.any(axis=1)
    assert zero.sum() > 0 and np.linalg.matrix_rank(D) <= D.shape[0] - zero.sum()
    sig = sc.sponge_sigma(13, sc.WIDTH, sc.sigma_max(lam))
    # (x and 1 - x of mirrored cells differ in the last bit, so the corners agree to rounding only)
    assert sig[6, 6] == 0.0 and sig[0, 0] == pytest.approx(sig.max(), rel=1e-14) and (sig == sig.T).all()
    assert 0.0 < sig.max() < sc.sigma_max(lam)
