"""CPU checks of the yardstick of the two-stage implicit Runge-Kutta steppers (lod_irk_cases.py) on the Q1 surrogate of
test_lod_harmonic_reference.py: nothing here calls the library.

  one-solve form  equals the undiagonalised stage system to 1e-11 of max |u| (measured <= 3.3e-13)
  modes           a mode x_j follows R(-lam_j dt)^k (heat) and the amplification matrix (wave) to 1e-10
  order           from halving dt twice on the lowest mode, at an end time that is no multiple of the period (the full
                  period superconverges): Gauss >= 3.8, Radau >= 2.7 (measured 4.00 and 2.90 - 2.98)
  stability       |R_radau(-lam_n 10 / lam_1)| < 1e-2 while Gauss's stays > 0.9: why both schemes exist
  growth          of the unpivoted complex LDL^T of every step matrix of the rule <= 1e4 (measured <= 1.5)
"""
import numpy as np
import pytest

import lod_irk_cases as ic

PENCILS = [(7, 1.0), (7, 1e4), (15, 1e4)]


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.parametrize("inner,contrast", PENCILS)
@pytest.mark.parametrize("label,scheme", ic.SCHEMES)
def test_one_solve_form_equals_the_stage_system(inner, contrast, label, scheme):
    A, M, lam, X = ic.q1_case(inner, contrast)
    n = A.shape[0]
    rng = np.random.default_rng(20251101 + scheme)
    u0, v0 = rng.standard_normal((n, 2)), rng.standard_normal((n, 2)) * np.sqrt(lam[0])
    steps, worst = 3, 0.0
    for dt in ic.heat_dts(lam):
        for loads in (None, rng.standard_normal((n, 2)) * lam[0], ic.stage_loads(rng, steps, (n, 2)) * lam[0]):
            worst = max(worst, _rel(ic.heat_one_solve(A, M, scheme, dt, steps, u0, loads),
                                    ic.heat_stage(A, M, scheme, dt, steps, u0, loads)))
    for dt in ic.wave_dts(lam):
        for _, dm, ds in ic.wave_dampings(lam):
            for loads in (None, ic.stage_loads(rng, steps, (n, 2)) * lam[0]):
                u1, v1 = ic.wave_one_solve(A, M, scheme, dt, steps, u0, v0, dm, ds, loads)
                u2, v2 = ic.wave_stage(A, M, scheme, dt, steps, u0, v0, dm, ds, loads)
                worst = max(worst, _rel(u1, u2), _rel(v1, v2))
    print("one-solve form against the stage system, %s, %d^2 nodes, contrast %g: %.2e" % (label, inner, contrast, worst))
    assert worst <= 1e-11


@pytest.mark.parametrize("label,scheme", ic.SCHEMES)
def test_modes_follow_the_stability_function(label, scheme):
    A, M, lam, X = ic.q1_case(7, 1e4)
    n, steps, worst = len(lam), 4, 0.0
    for j in (0, n // 2, n - 1):
        x = X[:, j]
        for dt in ic.heat_dts(lam):
            got = ic.heat_stage(A, M, scheme, dt, steps, x)
            R = ic.stability(scheme, -lam[j] * dt)
            want = np.array([R ** k * x for k in range(steps + 1)])
            worst = max(worst, _rel(got, want))
        for dt in ic.wave_dts(lam):
            for _, dm, ds in ic.wave_dampings(lam):
                w = np.sqrt(lam[j])
                us, vs = ic.wave_stage(A, M, scheme, dt, steps, x, w * x, dm, ds)
                G = ic.wave_amplification(scheme, dt, lam[j], dm, ds)
                y = np.array([1.0, w])
                for k in range(steps + 1):
                    worst = max(worst, float(np.abs(us[k] - y[0] * x).max() / np.abs(x).max()),
                                float(np.abs(vs[k] - y[1] * x).max() / (w * np.abs(x).max())))
                    y = G @ y
    print("modes against the stability function, %s: %.2e" % (label, worst))
    assert worst <= 1e-10


@pytest.mark.parametrize("label,scheme,least", [("gauss", ic.GAUSS, 3.8), ("radau", ic.RADAU, 2.7)])
def test_observed_order(label, scheme, least):
    A, M, lam, X = ic.q1_case(7, 1e4)
    x, w = X[:, 0], np.sqrt(lam[0])
    # heat: to t = 1 / lam_1; wave: 0.3 of a period, no multiple of it
    T_heat, T_wave = 1.0 / lam[0], 0.3 * 2.0 * np.pi / w
    eh, ew = [], []
    for steps in (2, 4, 8):
        eh.append(abs(ic.heat_stage(A, M, scheme, T_heat / steps, steps, x)[-1] @ (M @ x) - np.exp(-1.0)))
        us, _ = ic.wave_stage(A, M, scheme, T_wave / steps, steps, x, 0.0 * x)
        ew.append(abs(us[-1] @ (M @ x) - np.cos(w * T_wave)))
    for what, e in (("heat", eh), ("wave", ew)):
        orders = [float(np.log2(e[i] / e[i + 1])) for i in range(2)]
        print("observed order, %s, %s: %.2f %.2f (errors %.2e %.2e %.2e)" % (label, what, orders[0], orders[1], *e))
        assert min(orders) >= least, (what, orders)


def test_radau_damps_the_stiff_modes_and_gauss_does_not():
    for inner, contrast in PENCILS:
        lam = ic.q1_case(inner, contrast)[2]
        x = -lam[-1] * 10.0 / lam[0]
        assert abs(ic.stability(ic.RADAU, x)) < 1e-2
        assert abs(ic.stability(ic.GAUSS, x)) > 0.9


@pytest.mark.parametrize("inner,contrast", PENCILS)
def test_growth_of_every_step_matrix_stays_below_the_cap(inner, contrast):
    A, M, lam, X = ic.q1_case(inner, contrast)
    worst = 0.0
    for _, scheme in ic.SCHEMES:
        for dt in ic.heat_dts(lam):
            worst = max(worst, ic.growth(A, M, scheme, 1, dt)[0])
        for dt in ic.wave_dts(lam):
            for _, dm, ds in ic.wave_dampings(lam):
                worst = max(worst, ic.growth(A, M, scheme, 2, dt, dm, ds)[0])
    print("growth of the step matrices, %d^2 nodes, contrast %g: %.3f" % (inner, contrast, worst))
    assert worst <= ic.GROWTH_CAP
