"""CPU checks of the quad-precision oracle and of the yardstick built on it (tests/quad_cases.py).

The quad library is the truth the GPU parity tests of tests/test_gpu_quad_parity.py judge against, so it has to be
right for reasons that do not involve the device: its three selection algorithms (one-sided Jacobi on BD', Jacobi
eigen-solver on the Gram matrix, QR first) agree with each other five orders below the 1e-10 floor on every patch
(the certificate that the iterations are converged), every fp64 variant takes its decisions, and the bar derived
from it catches a stand-in for a kernel that loses three digits, which the bar derived from the oracle's spread
under a 1e-13 probe lets through.  Every test fails if the quad library cannot be built; none skips.

Measured here (e64_phi = what fp64 attains against the truth; min / median / max over the patches):
  Q1/D100  3.6e-14 / 1.5e-12 / 8.4e-11     largest bar max(1e-10, 10 spread) 5.5e-8 -> largest tol_phi 8.4e-10
  Q1/D1e4  2.6e-14 / 7.0e-12 / 1.7e-10     9.7e-8 -> 1.7e-9
  Q2/D1e4  5.0e-15 / 7.0e-12 / 2.2e-10     3.4e-8 -> 2.2e-9
  Q3/D1e4  4.4e-16 / 1.9e-15 / 2.0e-13     tol_phi = 1e-10 on every patch
  Q4/D1e4  1.3e-15 / 1.4e-14 / 6.1e-14     tol_phi = 1e-10 on every patch
"""
import numpy as np
import pytest

import quad_cases as qc

CERTIFICATE = 1e-15
IDS = ["%s-%s" % c for c in qc.CASES]


@pytest.mark.parametrize("case", qc.CASES, ids=IDS)
def test_certificate_three_quad_algorithms_agree(so, case):
    """Quad svd modes 0, 1 and 2 give phi and psi / ||A||_inf within 1e-15 of each other and equal decisions on every
    patch: the truth does not depend on how the singular triplets were computed.  On Q1 and Q2 most patches cut
    singular values, so the agreement covers the truncated pseudo-inverse and the 0.5 loop, not only d = -R^-1 c."""
    runs = [qc.quad_run(case, m) for m in (0, 1, 2)]
    pids = qc.all_patches(case)
    worst = 0.0
    for pid in pids:
        a_inf = qc.truth(case, pid)["a_inf"]
        phi0, psi0, dec0, _ = runs[0][pid]
        for m in (1, 2):
            phi, psi, dec, _ = runs[m][pid]
            e = max(np.abs(phi - phi0).max(), np.abs(psi - psi0).max() / a_inf)
            worst = max(worst, e)
            assert e <= CERTIFICATE, "patch %d: quad mode %d is %.3e from mode 0" % (pid, m, e)
            assert dec == dec0, "patch %d: quad mode %d decides %s, mode 0 %s" % (pid, m, dec, dec0)
    n_cut = sum(1 for pid in pids if any(d[0] > 0 for d in runs[0][pid][2]))
    n_drop = sum(1 for pid in pids if any(d[1] > 0 for d in runs[0][pid][2]))
    n_qr = sum(1 for pid in pids if runs[2][pid][3].sigma_max[0] == 0.0)
    print("%s-%s: %d patches, quad modes agree to %.1e; %d cut singular values, %d drop triplets in the 0.5 loop, "
          "mode 2 takes d = -R^-1 c on %d" % (case[0], case[1], len(pids), worst, n_cut, n_drop, n_qr))
    if case[0] in ("Q1", "Q2"):
        assert n_cut >= len(pids) // 2, "the configuration is meant to cut singular values on most patches"


@pytest.mark.parametrize("case", qc.CASES, ids=IDS)
def test_truth_differs_from_fp64_only_at_fp64_level(so, case):
    """The quad library is the same algorithm, not another one: the fp64 oracle is within 1e-9 of it everywhere (the
    largest fp64 error measured is 2.2e-10), and beyond the rounding of the result (> 1e-16) on some patch, i.e. the
    quad library is not the fp64 one under another name."""
    oracle = dict(qc.fp64_variants(case))["oracle"]
    errs = [float(np.abs(oracle[pid][0] - qc.truth(case, pid)["phi"]).max()) for pid in qc.all_patches(case)]
    assert max(errs) <= 1e-9, "fp64 oracle %.3e from the quad truth" % max(errs)
    assert max(errs) > 1e-16


@pytest.mark.parametrize("case", qc.CASES, ids=IDS)
def test_svd_mode_2_is_an_fp64_variant_like_the_others(so, case):
    """e64 takes the maximum over the variants, so a variant that is wrong would widen every bar.  The QR-first
    restatement is backward stable like the Jacobi on BD', so against the truth it may not be worse than ten times
    the worst of the other four variants on the same patch (floor 1e-13: below that the ratio is rounding of phi)."""
    variants = dict(qc.fp64_variants(case))
    worst = 0.0
    for pid in qc.all_patches(case):
        phi_q = qc.truth(case, pid)["phi"]
        e2 = float(np.abs(variants["svd_mode 2"][pid][0] - phi_q).max())
        others = max(float(np.abs(v[pid][0] - phi_q).max()) for n, v in variants.items() if n != "svd_mode 2")
        worst = max(worst, e2 / max(others, 1e-13))
        assert e2 <= 10.0 * max(others, 1e-13), "patch %d: svd_mode 2 %.3e, the other variants %.3e" % (pid, e2, others)
    print("%s-%s: svd_mode 2 against the truth is at most %.2f times the worst other variant" % (case[0], case[1], worst))


@pytest.mark.parametrize("case", qc.CASES, ids=IDS)
def test_nothing_left_out(so, case):
    """Every fp64 variant takes the truth's decisions on every patch the configuration keeps, and the patches taken
    out by id (quad_cases.DROPPED) are at most 5 % of it."""
    every = qc.all_patches(case)
    for pid in every:
        t = qc.truth(case, pid)
        if not t["asserted"]:
            print("patch %d: %s decide differently from the truth %s; margins of the truth: %.3e decades to the cutoff, "
                  "| ||d||_inf - 0.5 | = %.3e" % (pid, t["disagree"], t["decisions"], t["margin_cut"], t["margin_half"]))
    kept = qc.patches(case)
    assert len(every) - len(kept) <= 0.05 * len(every)
    left = [pid for pid in kept if not qc.decisions_asserted(case, pid)]
    assert not left, "decisions not shared by all fp64 variants on patches %s" % left


@pytest.mark.parametrize("case", [c for c in qc.CASES if c[0] in ("Q1", "Q2")], ids=lambda c: "%s-%s" % c)
def test_teeth_new_bar_sees_three_lost_digits(so, case):
    """The fp64 oracle with a relative noise of 1e-13 on X stands in for a kernel that loses three digits.  Against
    the fp64 oracle it stays inside max(1e-10, 10 * spread) on every patch; against the truth it breaks tol_phi on
    at least one patch."""
    cfg, fields = qc.setup(case)
    pids = qc.patches(case)
    clean = dict(qc.fp64_variants(case))["oracle"]
    so.set_solver_noise(1e-13)
    try:
        noisy = {pid: so.patch_basis(cfg, fields, pid)[0] for pid in pids}
    finally:
        so.set_solver_noise(0.0, 0)
    broken, worst_old = [], 0.0
    for pid in pids:
        bar = qc.old_bar(case, pid)[0]
        d_old = float(np.abs(noisy[pid] - clean[pid][0]).max())
        d_new = float(np.abs(noisy[pid] - qc.truth(case, pid)["phi"]).max())
        worst_old = max(worst_old, d_old / bar)
        assert d_old <= bar, "patch %d: the stand-in is %.3e from the fp64 oracle, outside the old bar %.3e" % (
            pid, d_old, bar)
        if d_new > qc.tol_phi(case, pid):
            broken.append(pid)
    print("%s-%s: stand-in uses at most %.2f of the old bar; it breaks tol_phi on %d of %d patches"
          % (case[0], case[1], worst_old, len(broken), len(pids)))
    assert broken, "the new bar lets a kernel that loses three digits through"


@pytest.mark.parametrize("case", qc.CASES, ids=IDS)
def test_e64_recorded(so, case):
    """Prints what fp64 attains against the truth (the lines of the table in DESIGN.md), and holds the yardstick to
    its own definition."""
    pids = qc.patches(case)
    e = np.array([qc.e64_phi(case, pid) for pid in pids])
    ep = np.array([qc.e64_psi(case, pid) for pid in pids])
    old = max(qc.old_bar(case, pid)[0] for pid in pids)
    new = max(qc.tol_phi(case, pid) for pid in pids)
    print("%s-%s: %d patches, e64_phi min %.2e median %.2e max %.2e; e64_psi/||A|| max %.2e; largest old bar %.2e, "
          "largest tol_phi %.2e" % (case[0], case[1], len(pids), e.min(), np.median(e), e.max(), ep.max(), old, new))
    for pid in pids:
        assert qc.tol_phi(case, pid) == max(1e-10, 10.0 * qc.e64_phi(case, pid))
        assert qc.tol_psi(case, pid) == max(1e-10, 10.0 * qc.e64_psi(case, pid)) * qc.truth(case, pid)["a_inf"]
    assert new <= old, "the bar from the truth is wider than the bar it replaces"


def test_quad_binding_and_margins(so):
    """slod_oracle.quad() offers the calls of the module bound to the quad library; its basis_many gives the words
    of its patch_basis; the margins are filled in both builds (finite where the SLOD branch decides, +inf where
    the LOD branch decides nothing)."""
    q = so.quad()
    kw = dict(nref=2, n_sub=2, oversampling=1, spacedim=1)
    cfg = q.make_cfg(**kw)
    from conftest import make_fields
    fields = make_fields(so, cfg, "D100")
    n = so.num_patches(cfg)
    sizes = [q.patch_info(cfg, pid).n_f for pid in range(n)]
    offs = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    phi, psi = q.basis_many(cfg, fields, np.arange(n), offs, int(sum(sizes)), nthreads=qc.nthreads())
    for pid in range(n):
        a, b, d = q.patch_basis(cfg, fields, pid)
        assert np.array_equal(phi[offs[pid]:offs[pid] + sizes[pid]], a.ravel())
        assert np.array_equal(psi[offs[pid]:offs[pid] + sizes[pid]], b.ravel())
        d64 = so.patch_basis(cfg, fields, pid)[2]
        for dd in (d, d64):
            assert 0.0 < dd.margin_cut[0] <= 15.0 and 0.0 < dd.margin_half[0] < np.inf
        dbg = q.patch_debug(cfg, fields, pid)
        assert np.abs(dbg["M"] - dbg["M"].T).max() <= 1e-15 * np.abs(dbg["M"]).max()
        st_q, st = q.assemble_patch(cfg, fields, pid), so.assemble_patch(cfg, fields, pid)
        assert np.abs(st_q - st).max() <= 8 * np.finfo(float).eps * np.abs(st).max()   # four element sums per entry
    lod = q.make_cfg(stabilize=0, **kw)
    d = q.patch_basis(lod, fields, 5)[2]
    assert d.margin_cut[0] == np.inf and d.margin_half[0] == np.inf
