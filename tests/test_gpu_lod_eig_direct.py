"""GPU tests of slod_lod_eigs_direct and slod_lod_eigs_ensemble_direct: block inverse iteration with Rayleigh-Ritz on
the pencil (A_LOD, M_LOD) with the inner solve on a banded Cholesky factor of S = A - sigma M, for one pencil and for the
pencils of a coefficient ensemble.

Single call, on the PENCIL_CONFIGS of lod_cases.py, with the bounds and the tol of test_gpu_lod_eig.py:
  eigenvalues        1e-8 relative against scipy.linalg.eigh(sym A, M)
  X^T M X = I        1e-10
  returned residual  against the one recomputed in numpy: 1e-6 relative, or both <= 1e-12 (full spectrum, the check of
                     test_gpu_lod_eig.py).  With guard columns the residuals stop near tol = 1e-10, where 1e-6 relative
                     is 1e-16 absolute: below the rounding of either evaluation of r = A x - theta M x, which cancels
                     to 1e-10 of its terms (measured: |res - recomputed| = 1.2e-16 at res = 6.6e-11).  There the bar is
                     1e-6 relative plus the first-order rounding bound of the two evaluations,
                     (n + cap s + m + 4) 2^-53 || |A||x| + |theta| |M||x| ||_2 / (|theta| ||M x||_2): n terms per entry
                     in numpy's product, cap s in the device's row product and m in its rotation by Q (Higham,
                     Accuracy and Stability, section 3.5), a few 1e-13 on these pencils.
  outer iterations   <= 2 ceil(log tol / log rho) + 5, rho = (lambda_{n_eig} - sigma) / (lambda_{m+1} - sigma)
  slod_lod_eigs      eigenvalues of the two solvers agree to 1e-8 relative
Ensemble call, on the three configurations of test_gpu_lod_ensemble_direct.py (members const / D100 / D1e4): every
comparison is one of 64-bit words against slod_lod_eigs_direct on the de-interleaved member.
The figures the tests print are recorded in DESIGN section 6, "Eigenpairs on banded Cholesky factors".
"""
import os
import re
import subprocess

import numpy as np
import pytest

import lod_eig_direct_cases as ed
from lod_cases import NAN, _bits, _build, _mass, _pencil, _symmetrize, _torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dealii-slod_amd", "bin", "main_Diffusion")
TOL = 1e-10


def _factor(c, sigma=0.0):
    S = ed.shifted(c.g, c.cols, c.sym, c.mvalues, sigma)
    return c.g.lod_factor(S.data_ptr(), c.cols.data_ptr())


def _direct(c, f, n_eig, m, **kw):
    return ed.eigs_direct(c.g, f, c.sym, c.mvalues, c.cols, c.nrow, n_eig, m, **kw)


def _residuals(c, X, theta):
    AX, MX = c.A @ X, c.M @ X
    return np.linalg.norm(AX - MX * theta, axis=0) / (np.abs(theta) * np.linalg.norm(MX, axis=0))


def _residual_floor(c, X, theta, m):
    """The rounding bound of the two evaluations of the normalised residual (module docstring), per column."""
    terms = c.nrow + c.g.lod_row_capacity() * c.s + m + 4
    mag = np.abs(c.A) @ np.abs(X) + (np.abs(c.M) @ np.abs(X)) * np.abs(theta)
    return terms * 2.0 ** -53 * np.linalg.norm(mag, axis=0) / (np.abs(theta) * np.linalg.norm(c.M @ X, axis=0))


def _block_width(lam, n_eig):
    """The smallest m >= n_eig with rho = lambda_{n_eig} / lambda_{m+1} <= 0.5, as test_gpu_lod_eig.py chooses it."""
    for m in range(n_eig, len(lam) + 1):
        if ed.contraction(lam, n_eig, m) <= 0.5:
            return m
    raise AssertionError("unreachable")


# ---- the single call

@pytest.mark.parametrize("name", ["s1", "rowmajor", "s2", "step64"])
def test_full_spectrum_matches_dense(so, name):
    c = _pencil(so, name)
    m = c.nrow
    assert m == {"s1": 16, "rowmajor": 25, "s2": 32, "step64": 64}[name]
    f = _factor(c)
    lam, res, outer, X = _direct(c, f, m, m)
    f.close()
    hX = X.cpu().numpy()
    err = np.abs(lam / c.lam - 1.0).max()
    orth = np.abs(hX.T @ c.M @ hX - np.eye(m)).max()
    ref = _residuals(c, hX, lam)
    print("%s m = rows = %d: outer %d, max eigenvalue error %.3e (bound 1e-8), max |X^T M X - I| %.3e (bound 1e-10), "
          "residuals max %.3e (recomputed %.3e)" % (name, m, outer, err, orth, res.max(), ref.max()))
    assert (np.diff(lam) >= 0).all()
    assert err <= 1e-8
    assert orth <= 1e-10
    for j in range(m):
        assert abs(res[j] - ref[j]) <= 1e-6 * ref[j] or (res[j] <= 1e-12 and ref[j] <= 1e-12), (j, res[j], ref[j])


@pytest.mark.parametrize("n_eig", [1, 2, 6])
@pytest.mark.parametrize("name", ["step64", "const"])
def test_lowest_pairs_with_guards_and_agreement_with_cg(so, name, n_eig):
    torch, dev = _torch()
    c = _pencil(so, name)
    m = _block_width(c.lam, n_eig)
    rho = ed.contraction(c.lam, n_eig, m)
    f = _factor(c)
    lam, res, outer, X = _direct(c, f, n_eig, m)
    f.close()
    hX = X.cpu().numpy()
    err = np.abs(lam[:n_eig] / c.lam[:n_eig] - 1.0).max()
    orth = np.abs(hX.T @ c.M @ hX - np.eye(m)).max()
    ref = _residuals(c, hX, lam)
    Xc = torch.full((c.nrow, m), NAN, dtype=torch.float64, device=dev)
    lam_cg, res_cg, its = c.g.lod_eigs(c.sym.data_ptr(), c.mvalues.data_ptr(), c.cols.data_ptr(), n_eig, Xc.data_ptr(), n_block=m)
    agree = np.abs(lam[:n_eig] / lam_cg[:n_eig] - 1.0).max()
    bound = ed.outer_bound(rho, TOL)
    print("%s n_eig %d, m %d, rho %.3f: outer %d (bound %d; slod_lod_eigs %d), eigenvalue error %.3e, |X^T M X - I| %.3e, "
          "residuals %s, against slod_lod_eigs %.3e" % (name, n_eig, m, rho, outer, bound, len(its), err, orth,
                                                        ["%.2e" % r for r in res[:n_eig]], agree))
    assert err <= 1e-8
    assert orth <= 1e-10
    assert (res[:n_eig] <= TOL).all()
    assert outer <= bound
    assert agree <= 1e-8
    floor = _residual_floor(c, hX, lam, m)
    print("   |res - recomputed| max %.3e, rounding floor min %.3e" % (np.abs(res - ref)[:n_eig].max(), floor[:n_eig].min()))
    for j in range(n_eig):
        assert abs(res[j] - ref[j]) <= 1e-6 * ref[j] + floor[j], (j, res[j], ref[j], floor[j])


@pytest.mark.parametrize("name,n_eig,m", [("step64", 2, 4), ("const", 2, 4)])
def test_outer_iterations_within_the_bound_with_and_without_a_shift(so, name, n_eig, m):
    c = _pencil(so, name)
    sigma = 0.9 * c.lam[0]
    rho0, rho1 = ed.contraction(c.lam, n_eig, m), ed.contraction(c.lam, n_eig, m, sigma)
    b0, b1 = ed.outer_bound(rho0, TOL), ed.outer_bound(rho1, TOL)
    assert b1 < b0, (rho0, rho1, b0, b1)                              # on the CPU first: the case separates the two bounds
    runs = []
    for s in (0.0, sigma):
        f = _factor(c, s)
        lam, res, outer, X = _direct(c, f, n_eig, m)
        f.close()
        assert np.abs(lam[:n_eig] / c.lam[:n_eig] - 1.0).max() <= 1e-8 and (res[:n_eig] <= TOL).all()
        runs.append(outer)
    print("%s n_eig %d, m %d: sigma 0: rho %.3f, outer %d (bound %d); sigma 0.9 lambda_1: rho %.3f, outer %d (bound %d)"
          % (name, n_eig, m, rho0, runs[0], b0, rho1, runs[1], b1))
    assert runs[0] <= b0 and runs[1] <= b1
    assert runs[1] <= runs[0]


@pytest.mark.parametrize("m,n_eig", [(1, 1), (2, 2), (2, 1), (5, 3), (5, 5), (17, 4), (17, 17), (64, 8), (64, 64)])
def test_block_shapes_padding_and_repeatability(so, m, n_eig):
    """n_block 1, 2, odd, across the 16-column tile of the factor solve and the cap, n_eig = and < n_block; the caller's
    start block in a padded ld_x whose NaN padding stays; a repeated call equal as 64-bit words."""
    c = _pencil(so, "step64")
    f = _factor(c)
    lam, res, outer, X = _direct(c, f, n_eig, m)
    print("step64 m %d n_eig %d: outer %d, eigenvalue error %.3e, residuals max %.3e" %
          (m, n_eig, outer, np.abs(lam[:n_eig] / c.lam[:n_eig] - 1.0).max(), res[:n_eig].max()))
    assert np.isfinite(lam).all() and np.isfinite(res).all() and bool(_torch()[0].isfinite(X).all())
    assert 1 <= outer <= 200
    if outer < 200:                                                  # (a block that ends inside a cluster may not get there)
        assert (res[:n_eig] <= TOL).all() and np.abs(lam[:n_eig] / c.lam[:n_eig] - 1.0).max() <= 1e-8
        hX = X.cpu().numpy()
        assert np.abs(hX.T @ c.M @ hX - np.eye(m)).max() <= 1e-10
    # the caller's block in a padded ld_x, twice
    X0 = np.random.default_rng(41).uniform(-1.0, 1.0, (c.nrow, m))
    runs = [_direct(c, f, n_eig, m, X0=X0, ld=m + 3) for _ in range(2)]
    f.close()
    (l0, r0, o0, x0), (l1, r1, o1, x1) = runs
    torch, dev = _torch()
    assert bool(torch.isnan(x0[:, m:]).all()) and bool(torch.isfinite(x0[:, :m]).all())
    assert ed.same_words(l0, l1) and ed.same_words(r0, r1) and o0 == o1
    assert np.array_equal(_bits(x0[:, :m]), _bits(x1[:, :m]))


def test_max_outer_one_is_a_result(so):
    c = _pencil(so, "step64")
    f = _factor(c)
    lam, res, outer, X = _direct(c, f, 2, 8, max_outer=1)
    f.close()
    assert outer == 1
    assert np.isfinite(res).all() and np.isfinite(lam).all() and np.isfinite(X.cpu().numpy()).all()
    assert not (res[:2] <= TOL).all()                                # one iteration from the sine block does not converge


def test_rank_deficient_start_block_and_refusals(so):
    import slod_amd
    torch, dev = _torch()
    c = _pencil(so, "step64")
    m, n_eig = 6, 2
    f = _factor(c)
    X0 = np.random.default_rng(43).uniform(-1.0, 1.0, (c.nrow, m))
    X0[:, m - 1] = X0[:, 0]                                          # two equal columns: Gm = Z^T M Z is singular
    X = ed._nan(c.nrow, m + 2)
    X[:, :m] = ed._dev(X0)
    before = _bits(X).copy()
    with pytest.raises(slod_amd.SlodError) as e:
        c.g.lod_eigs_direct(f, c.sym.data_ptr(), c.mvalues.data_ptr(), c.cols.data_ptr(), n_eig, X.data_ptr(), n_block=m, ld_x=m + 2,
                            start=1)
    print("rank-deficient block:", e.value)
    assert e.value.code == -5 and "pivot" in str(e.value) and "slod_lod_eigs_direct" in str(e.value)
    assert "outer iteration 1" in str(e.value)
    assert np.array_equal(_bits(X), before)                          # d_x holds the start block, the padding its NaN
    # wherever the copy of column 0 stands, and whatever the sign of the rounding left in its pivot
    for seed in (43, 53):
        for width in (2, 5):
            for j in range(1, width):
                Xj = np.random.default_rng(seed).uniform(-1.0, 1.0, (c.nrow, width))
                Xj[:, j] = Xj[:, 0]
                with pytest.raises(slod_amd.SlodError) as e:
                    _direct(c, f, 1, width, X0=Xj, max_outer=1)
                assert e.value.code == -5, (seed, width, j)
    # the refusals that need a factor
    e3 = ed.ensemble_case(so, "base")                                # 64 rows as step64, another handle
    V = ed.stack(e3, e3.sym, 3)
    f3 = e3.g.lod_factor_ensemble(V.data_ptr(), e3.cols.data_ptr(), 3)
    a0, m0 = e3.sym[0], e3.mass[0]
    Y = ed._nan(e3.nrow, m)
    with pytest.raises(slod_amd.SlodError) as e:                     # a factor of three members
        e3.g.lod_eigs_direct(f3, a0.data_ptr(), m0.data_ptr(), e3.cols.data_ptr(), n_eig, Y.data_ptr(), n_block=m)
    assert e.value.code == -1 and "slod_lod_eigs_direct: factor of another member count" in str(e.value)
    with pytest.raises(slod_amd.SlodError) as e:                     # the factor of another handle
        e3.g.lod_eigs_direct(f, a0.data_ptr(), m0.data_ptr(), e3.cols.data_ptr(), n_eig, Y.data_ptr(), n_block=m)
    assert e.value.code == -1 and "slod_lod_eigs_direct: factor of another handle" in str(e.value)
    small = _pencil(so, "s1")                                        # 16 rows: another row count, and another handle
    with pytest.raises(slod_amd.SlodError) as e:
        small.g.lod_eigs_direct(f, small.sym.data_ptr(), small.mvalues.data_ptr(), small.cols.data_ptr(), n_eig, Y.data_ptr(), n_block=m)
    assert e.value.code == -1 and "factor of another handle" in str(e.value)
    assert bool(torch.isnan(Y).all())                                # nothing was written
    f3.close()
    f.close()


# ---- the ensemble call

def _ensemble_equals_singles(c, K, n_eig, m, tol=TOL, max_outer=200, pad_a=1, pad_m=2, pad_x=3):
    """One ensemble call from the sine block (padded leading dimensions, NaN in every padding) against the K single
    calls; returns the member counts."""
    torch, dev = _torch()
    A, M = ed.stack(c, c.sym, K, pad=pad_a), ed.stack(c, c.mass, K, pad=pad_m)
    f = c.g.lod_factor_ensemble(A.data_ptr(), c.cols.data_ptr(), K, ld_m=K + pad_a)
    lam, res, status, rc, X = ed.eigs_ensemble(c.g, f, A, M, c.cols, c.nrow, K, n_eig, m, ld=K * m + pad_x, ld_a_m=K + pad_a,
                                               ld_m_m=K + pad_m, tol=tol, max_outer=max_outer)
    f.close()
    assert rc == status.max() and (status >= 1).all()
    assert bool(torch.isnan(X[:, K * m:]).all()) and bool(torch.isfinite(X[:, :K * m]).all())
    assert bool(torch.isnan(A[:, K:]).all()) and bool(torch.isnan(M[:, K:]).all())
    xb = _bits(X)
    singles = ed.member_singles(c, A, M, K, n_eig, m, tol=tol, max_outer=max_outer)
    for k, (l1, r1, o1, x1) in enumerate(singles):
        assert status[k] == o1, (c.name, K, m, k, status[k], o1)
        assert ed.same_words(lam[k], l1) and ed.same_words(res[k], r1), (c.name, K, m, k)
        assert np.array_equal(xb[:, k * m:(k + 1) * m], x1), (c.name, K, m, k)
    return status, res


@pytest.mark.parametrize("m", [1, 5, 17])
@pytest.mark.parametrize("name", ed.NAMES)
def test_ensemble_of_three_equals_single_calls(so, name, m):
    c = ed.ensemble_case(so, name)
    n_eig = min(m, 3)
    status, res = _ensemble_equals_singles(c, c.K, n_eig, m)
    print("%s K = 3, m = %d, n_eig = %d: outer per member %s, residuals max %s"
          % (name, m, n_eig, status.tolist(), ["%.2e" % r for r in res[:, :n_eig].max(axis=1)]))


@pytest.mark.parametrize("m", [1, 5, 17])
def test_ensemble_of_65_scaled_copies_equals_single_calls(so, m):
    c = ed.ensemble_case(so, "base")
    n_eig = min(m, 3)
    status, _ = _ensemble_equals_singles(c, 65, n_eig, m)
    print("base K = 65, m = %d: outer per member min %d max %d" % (m, status.min(), status.max()))


def _model_counts(c, n_eig, m, tol):
    X0 = ed.sine_block(c.g, c.s, m)
    return [ed.model_eigs(c.A[k], c.M[k], X0, n_eig, tol)[2] for k in range(c.K)]


def test_members_stop_on_their_own(so):
    """The freeze really runs: tol is chosen on the numpy model so that const and D1e4 need counts that differ by two or
    more, then the device counts must differ too (and equal the single calls', which stop on the host's comparison)."""
    c = ed.ensemble_case(so, "base")
    chosen = None
    for n_eig, m in ((3, 5), (1, 1), (2, 3), (1, 2)):
        for tol in (1e-10, 1e-8, 1e-6, 1e-4):
            counts = _model_counts(c, n_eig, m, tol)
            print("model: n_eig %d, m %d, tol %.0e: outer per member %s" % (n_eig, m, tol, counts))
            if chosen is None and abs(counts[0] - counts[2]) >= 2 and max(counts) < 100:
                chosen = (n_eig, m, tol, counts)
    assert chosen is not None
    n_eig, m, tol, counts = chosen
    status, res = _ensemble_equals_singles(c, c.K, n_eig, m, tol=tol)
    print("device: tol %.0e: outer per member %s (model %s)" % (tol, status.tolist(), counts))
    assert status[0] != status[2]
    assert (res[:, :n_eig] <= tol).all()
    # max_outer below the slowest member's count: the fast members are done, the slow one is not, and that is no error
    fast, slow = int(status.min()), int(status.max())
    cut = slow - 1
    assert fast <= cut
    status2, res2 = _ensemble_equals_singles(c, c.K, n_eig, m, tol=tol, max_outer=cut)
    assert [int(v) for v in status2] == [min(int(v), cut) for v in status]
    for k in range(c.K):
        assert bool((res2[k, :n_eig] <= tol).all()) == (status[k] <= cut), k


def test_ensemble_is_independent_of_position_padding_and_the_other_members(so):
    torch, dev = _torch()
    c = ed.ensemble_case(so, "rowmajor")
    K, n_eig, m = c.K, 2, 5
    X0 = np.random.default_rng(47).uniform(-1.0, 1.0, (c.nrow, K * m))       # a start block that differs per member
    A, M = ed.stack(c, c.sym, K), ed.stack(c, c.mass, K)
    f = c.g.lod_factor_ensemble(A.data_ptr(), c.cols.data_ptr(), K)
    lam, res, status, rc, X = ed.eigs_ensemble(c.g, f, A, M, c.cols, c.nrow, K, n_eig, m, X0=X0)
    f.close()
    ref = _bits(X)
    singles = ed.member_singles(c, A, M, K, n_eig, m, X0=X0)
    for k, (l1, r1, o1, x1) in enumerate(singles):
        assert status[k] == o1 and ed.same_words(lam[k], l1) and ed.same_words(res[k], r1)
        assert np.array_equal(ref[:, k * m:(k + 1) * m], x1), k
    assert not np.array_equal(ref[:, :m], ref[:, m:2 * m])
    # permuted members, ld_a_m != ld_m_m and a padded ld_x, NaN in every padding
    perm = [2, 0, 1]
    tp = torch.tensor(perm, device=dev)
    Ap, Mp = ed._nan(c.nval, K + 1), ed._nan(c.nval, K + 4)
    Ap[:, :K], Mp[:, :K] = A[:, tp], M[:, tp]
    X0p = np.concatenate([X0[:, p * m:(p + 1) * m] for p in perm], axis=1)
    f = c.g.lod_factor_ensemble(Ap.data_ptr(), c.cols.data_ptr(), K, ld_m=K + 1)
    lam2, res2, status2, rc2, X2 = ed.eigs_ensemble(c.g, f, Ap, Mp, c.cols, c.nrow, K, n_eig, m, X0=X0p, ld=K * m + 7,
                                                    ld_a_m=K + 1, ld_m_m=K + 4)
    f.close()
    assert bool(torch.isnan(X2[:, K * m:]).all()) and bool(torch.isnan(Ap[:, K:]).all()) and bool(torch.isnan(Mp[:, K:]).all())
    got = _bits(X2)
    for i, p in enumerate(perm):
        assert status2[i] == status[p] and ed.same_words(lam2[i], lam[p]) and ed.same_words(res2[i], res[p])
        assert np.array_equal(got[:, i * m:(i + 1) * m], ref[:, p * m:(p + 1) * m]), (i, p)
    assert rc2 == rc


def test_one_member_with_a_rank_deficient_block(so):
    import slod_amd
    torch, dev = _torch()
    c = ed.ensemble_case(so, "base")
    K, n_eig, m = c.K, 2, 5
    X0 = np.random.default_rng(53).uniform(-1.0, 1.0, (c.nrow, K * m))
    X0[:, m + m - 1] = X0[:, m]                                      # member 1: two equal columns (its last and its first)
    A, M = ed.stack(c, c.sym, K), ed.stack(c, c.mass, K)
    f = c.g.lod_factor_ensemble(A.data_ptr(), c.cols.data_ptr(), K)
    lam, res, status, rc, X = ed.eigs_ensemble(c.g, f, A, M, c.cols, c.nrow, K, n_eig, m, X0=X0, check=False)
    msg = c.g.lib.slod_last_error(c.g.h).decode()
    print("one bad member: rc %d, member_status %s, %s" % (rc, status.tolist(), msg))
    assert rc == -5 and status[1] == -5 and status[0] >= 1 and status[2] >= 1
    assert "slod_lod_eigs_ensemble_direct" in msg and "member 1" in msg and "outer iteration 1" in msg
    xb = _bits(X)
    assert np.array_equal(xb[:, m:2 * m], X0[:, m:2 * m].view(np.uint64))        # member 1 keeps its start block
    with pytest.raises(slod_amd.SlodError) as e:
        ed.eigs_ensemble(c.g, f, A, M, c.cols, c.nrow, K, n_eig, m, X0=X0)
    assert e.value.code == -5
    f.close()
    singles = ed.member_singles(c, A[:, [0, 2]].contiguous(), M[:, [0, 2]].contiguous(), 2, n_eig, m,
                                X0=np.concatenate([X0[:, :m], X0[:, 2 * m:]], axis=1))
    for (l1, r1, o1, x1), k in zip(singles, (0, 2)):
        assert status[k] == o1 and ed.same_words(lam[k], l1) and ed.same_words(res[k], r1), k
        assert np.array_equal(xb[:, k * m:(k + 1) * m], x1), k


def test_ensemble_refuses_a_factor_of_another_member_count(so):
    import slod_amd
    c = ed.ensemble_case(so, "rowmajor")
    K, m = c.K, 4
    A, M = ed.stack(c, c.sym, K), ed.stack(c, c.mass, K)
    f3 = c.g.lod_factor_ensemble(A.data_ptr(), c.cols.data_ptr(), K)
    f1 = c.g.lod_factor(c.sym[0].data_ptr(), c.cols.data_ptr())
    X = ed._nan(c.nrow, K * m)
    for fac, members in ((f3, K - 1), (f1, K)):
        with pytest.raises(slod_amd.SlodError) as e:
            c.g.lod_eigs_ensemble_direct(fac, A.data_ptr(), M.data_ptr(), c.cols.data_ptr(), members, 2, X.data_ptr(), n_block=m,
                                         ld_a_m=K, ld_m_m=K, ld_x=K * m)
        assert e.value.code == -1 and "slod_lod_eigs_ensemble_direct: factor of another member count" in str(e.value)
    assert bool(_torch()[0].isnan(X).all())
    f1.close()
    f3.close()


def test_pipeline_equals_three_single_pipelines(so):
    """plan -> A, M of the ensemble -> sym -> factor -> eigs_ensemble_direct -> reconstruction of the first eigenvector,
    against the three single pipelines, word for word."""
    torch, dev = _torch()
    c = ed.ensemble_case(so, "base")
    g, K, n_eig, m = c.g, c.K, 2, 6
    V, M, A = ed._nan(c.nval, K), ed._nan(c.nval, K), ed._nan(c.nval, K)
    cols, mcols = torch.zeros_like(c.cols), torch.zeros_like(c.cols)
    torch.cuda.synchronize()
    g.lod_matrix_ensemble(c.b.data_ptr(), c.q.data_ptr(), c.stride, K, V.data_ptr(), cols.data_ptr())
    g.lod_mass_matrix_ensemble(c.b.data_ptr(), c.stride, K, M.data_ptr(), mcols.data_ptr())
    g.lod_matrix_symmetrize_ensemble(V.data_ptr(), cols.data_ptr(), K, A.data_ptr())
    f = g.lod_factor_ensemble(A.data_ptr(), cols.data_ptr(), K)
    lam, res, status, rc, X = ed.eigs_ensemble(g, f, A, M, cols, c.nrow, K, n_eig, m)
    f.close()
    first = X[:, ::m].contiguous()                                   # column 0 of every member: [nrow][K]
    fine = ed._nan(K, c.field)
    g.lod_reconstruct_ensemble(c.b.data_ptr(), c.stride, K, first.data_ptr(), fine.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(cols, c.cols) and torch.equal(mcols, c.cols)
    for k in range(K):
        fk = g.lod_factor(c.sym[k].data_ptr(), c.cols.data_ptr())
        l1, r1, o1, x1 = ed.eigs_direct(g, fk, c.sym[k], c.mass[k], c.cols, c.nrow, n_eig, m)
        fk.close()
        assert status[k] == o1 and ed.same_words(lam[k], l1) and ed.same_words(res[k], r1), k
        assert np.array_equal(_bits(X[:, k * m:(k + 1) * m]), _bits(x1)), k
        u = x1[:, :1].contiguous()
        out = ed._nan(c.field)
        g.lod_reconstruct(c.slab[k][0].data_ptr(), c.stride, u.data_ptr(), out.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(_bits(fine[k]), _bits(out)), k
        assert (res[k, :n_eig] <= TOL).all()
    print("pipeline: lambda_1 per member %s, outer %s" % (lam[:, 0].tolist(), status.tolist()))
    assert len({float(v) for v in lam[:, 0]}) == K                   # the members differ


# ---- the driver

def _driver(*args):
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "dealii-slod_amd"), "bin/main_Diffusion"])
    r = subprocess.run([BIN, "3", "4", "1", "1", *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return r.stdout


def test_driver_eigs_direct_matches_python_path(so):
    out = _driver("--eigs", "4", "--direct")
    pairs = re.findall(r"^eigenvalue (\d+) = (\S+), residual = (\S+)$", out, re.M)
    assert [int(p[0]) for p in pairs] == [1, 2, 3, 4], out
    d_lam, d_res = np.array([float(p[1]) for p in pairs]), np.array([float(p[2]) for p in pairs])
    counts = re.search(r"^eigensolver: outer iterations = (\d+), direct$", out, re.M)
    assert counts, out
    factor = re.findall(r"^factor: n = (\d+), half bandwidth = (\d+), bytes = (\d+), pivots in \[(\S+), (\S+)\]$", out, re.M)
    assert len(factor) == 1 and factor[0][:2] == ("64", "27") and float(factor[0][3]) > 0.0, out
    assert "inner iterations" not in out
    torch, dev = _torch()
    cfg = so.make_cfg(nref=3, n_sub=4, oversampling=1, stabilize=1)
    c = _build(so, dict(nref=3, n_sub=4, oversampling=1, spacedim=1),
               fields=[so.fill_coefficient_rand(1.0, 100.0, 3, so.n_cells_per_side(cfg) * 4, seed=1)])
    c.mvalues, _ = _mass(c)
    c.sym = _symmetrize(c)
    f = c.g.lod_factor(c.sym.data_ptr(), c.cols.data_ptr())
    X = torch.full((c.nrow, 8), NAN, dtype=torch.float64, device=dev)
    lam, res, outer = c.g.lod_eigs_direct(f, c.sym.data_ptr(), c.mvalues.data_ptr(), c.cols.data_ptr(), 4, X.data_ptr())
    f.close()
    print("driver eigenvalues", d_lam, "python", lam[:4], "outer", counts.group(1), outer)
    assert len(lam) == 8
    assert np.abs(d_lam / lam[:4] - 1.0).max() <= 1e-8
    assert int(counts.group(1)) == outer
    assert (d_res <= TOL).all() and (res[:4] <= TOL).all()
    # a shift below lambda_1 gives the same eigenvalues
    shifted = _driver("--eigs", "4", "--direct", "--shift", repr(0.5 * float(lam[0])))
    s_lam = np.array([float(p[1]) for p in re.findall(r"^eigenvalue (\d+) = (\S+), residual = (\S+)$", shifted, re.M)])
    assert len(s_lam) == 4 and np.abs(s_lam / lam[:4] - 1.0).max() <= 1e-8


def test_driver_ensemble_eigs_direct():
    """--ensemble 3 --eigs 2 --direct prints per member what three --member k --eigs 2 --direct runs print, to the digits
    printed, and the mean and standard deviation of each eigenvalue over the members."""
    K, N = 3, 2
    out = _driver("--ensemble", str(K), "--eigs", str(N), "--direct")
    lines = re.findall(r"^member (\d+) eigenvalue (\d+) = (\S+), residual = (\S+)$", out, re.M)
    assert [(int(a), int(b)) for a, b, _, _ in lines] == [(k, j) for k in range(K) for j in range(1, N + 1)], out
    outer = dict(re.findall(r"^member (\d+) eigensolver: outer iterations = (\d+), direct$", out, re.M))
    assert sorted(outer) == ["0", "1", "2"], out
    stats = re.findall(r"^eigenvalue (\d+) over the ensemble of 3: mean = (\S+), standard deviation = (\S+)$", out, re.M)
    assert [int(s[0]) for s in stats] == [1, 2], out
    vals = {}
    for k in range(K):
        one = _driver("--member", str(k), "--eigs", str(N), "--direct")
        pairs = re.findall(r"^eigenvalue (\d+) = (\S+), residual = (\S+)$", one, re.M)
        cnt = re.search(r"^eigensolver: outer iterations = (\d+), direct$", one, re.M)
        assert len(pairs) == N and cnt, one
        for j, lam, res in pairs:
            got = [(l, r) for a, b, l, r in lines if (int(a), int(b)) == (k, int(j))][0]
            assert got == (lam, res), (k, j, got, lam, res)
            vals[(k, int(j))] = float(lam)
        assert outer[str(k)] == cnt.group(1), k
    for j, mean, std in stats:
        x = np.array([vals[(k, int(j))] for k in range(K)])
        assert abs(float(mean) / x.mean() - 1.0) <= 1e-6 and abs(float(std) / x.std(ddof=1) - 1.0) <= 1e-5, (j, mean, std)
        assert float(std) > 0.0                                      # the members differ
