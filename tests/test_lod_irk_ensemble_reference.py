"""CPU checks of the rule for dt of the ensemble implicit Runge-Kutta tests (lod_irk_ensemble_cases.py), before the GPU
test relies on it: on the Q1 surrogate pencils of lod_irk_cases.q1_case at contrasts 1, 100 and 1e4 as three members, at
the joint rule (lam_1 := max_k lam_1(k), lam_n := max_k lam_n(k)) every member's step matrix has growth <= GROWTH_CAP, the
project's condition before the library is called, for heat and for wave with every damping; and the scaled copies
(1 + k/64) (A, M) of the K = 65 ensemble have the growth of their member.  Nothing here calls the library."""
import numpy as np
import pytest

import lod_irk_cases as ic
import lod_irk_ensemble_cases as ec


def test_joint_rule_is_the_rule_on_the_joint_spectrum():
    members = ec.surrogate_members()
    lams = [m[2] for m in members]
    l1, ln = max(l[0] for l in lams), max(l[-1] for l in lams)
    assert ec.heat_dts(lams) == [0.1 / l1, 1.0 / np.sqrt(l1 * ln), 10.0 / l1]
    assert ec.wave_dts(lams) == [0.5 / np.sqrt(l1), 0.05 / np.sqrt(l1), 2.0 / np.sqrt(ln)]
    # the stiffest member sets the step: no member's rule gives a smaller one at either end
    for l in lams:
        assert ec.heat_dts(lams)[0] <= ic.heat_dts(l)[0] and ec.wave_dts(lams)[2] <= ic.wave_dts(l)[2]
    labels = [p[0] for p in ec.problems(lams)]
    assert labels == ["heat", "wave-none", "wave-mass", "wave-stiff", "wave-both"]


@pytest.mark.parametrize("label,scheme", ic.SCHEMES)
def test_every_member_keeps_the_growth_cap_at_the_joint_rule(label, scheme):
    members = ec.surrogate_members()
    lams = [m[2] for m in members]
    worst = 0.0
    for plabel, order, dts, dm, ds in ec.problems(lams):
        for dt in dts:
            for k, (A, M, _) in enumerate(members):
                g, _ = ic.growth(A, M, scheme, order, dt, dm, ds)
                worst = max(worst, g)
                assert g <= ic.GROWTH_CAP, (label, plabel, dt, k, g)
    print("%s: largest growth of a member's step matrix at the joint rule %.3f" % (label, worst))


@pytest.mark.parametrize("label,scheme", ic.SCHEMES)
def test_scaled_copies_have_the_growth_of_their_member(label, scheme):
    members = ec.surrogate_members()
    lams = [m[2] for m in members]
    K = 65
    for plabel, order, dts, dm, ds in ec.problems(lams):
        dt = dts[1]
        own = [ic.growth(A, M, scheme, order, dt, dm, ds)[0] for A, M, _ in members]
        for k in (3, 4, 5, 31, 64):
            f = ec.scale(K, k)
            assert f == 1.0 + k / 64.0
            A, M, _ = members[k % 3]
            g, _ = ic.growth(A * f, M * f, scheme, order, dt, dm, ds)
            assert g <= ic.GROWTH_CAP and abs(g - own[k % 3]) <= 1e-10 * own[k % 3], (label, plabel, k, g, own[k % 3])
    assert [ec.scale(K, k) for k in range(3)] == [1.0, 1.0, 1.0]
