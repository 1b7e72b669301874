"""GPU tests of slod_lod_eigs_shift_direct and slod_lod_eigs_shift_ensemble_direct: the eigenpairs of (A_LOD, M_LOD)
nearest a shift sigma inside the spectrum, by block inverse iteration on the banded LDL^T factor of
S = sym(A) - sigma M with the Ritz pairs ordered by their distance from sigma.

Pencils: step64 (64 rows), s2 (elasticity, 128 rows), morton16 (256 rows) of lod_ldl_cases.py, each with
sigma = shift_at(.., rows / 4) and shift_at(.., rows / 2); n_eig = 4, n_block = 8, tol = 1e-10.
Bars, those of test_gpu_lod_eig_direct.py:
  eigenvalues        1e-8 relative against the n_eig of scipy's spectrum nearest sigma, in order of distance (the two
                     nearest a gap's midpoint are equidistant up to rounding: _nearest_error)
  X^T M X = I        1e-10
  returned residual  <= tol, and against numpy's recomputation 1e-6 relative plus the rounding floor of that file
  outer iterations   <= 2 ceil(log tol / log rho) + 5, rho = |lambda_(n_eig) - sigma| / |lambda_(m+1) - sigma| with the
                     eigenvalues in order of distance from sigma; the numpy model (lod_eig_direct_cases.model_eigs with
                     the distance ordering, below) is run first and must stay inside the bound itself
  inertia            the converged eigenvalues below sigma are never more than n_negative of the factor; on the 16-row
                     case with the full spectrum they are exactly n_negative
  words              start = 0 starts from the hash of include/slod.h; two calls agree; every ensemble member has the
                     words of the single call on its de-interleaved data
"""
import os
import re
import subprocess

import numpy as np
import pytest

import lod_eig_direct_cases as ed
import lod_ldl_cases as lc
from lod_cases import NAN, _bits, _build, _mass, _rows_to_dense, _symmetrize, _torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dealii-slod_amd", "bin", "main_Diffusion")
TOL = 1e-10
N_EIG, M_BLOCK = 4, 8
PENCILS = ("step64", "s2", "morton16")
SEED = 401                                   # of the caller's start block of the outer-count test


def _nearest(lam, sigma):
    """The indices of lam in order of |lam - sigma|, ties by ascending lam (lam is ascending: a stable sort)."""
    return np.argsort(np.abs(lam - sigma), kind="stable")


def _nearest_error(got, spectrum, sigma):
    """The returned eigenvalues against the len(got) of the spectrum nearest sigma, in order of distance.  A shift of
    shift_at is the midpoint of a gap, so the two nearest eigenvalues are equidistant from it up to rounding and either
    may come first: the distances are compared in order, |got_j - sigma| with |want_j - sigma|, and the values as sets
    (both sorted ascending), each relative to the eigenvalue.  Returns the larger of the two errors."""
    want = spectrum[_nearest(spectrum, sigma)[:len(got)]]
    by_distance = np.abs(np.abs(got - sigma) - np.abs(want - sigma)) / np.abs(want)
    by_value = np.abs(np.sort(got) / np.sort(want) - 1.0)
    return max(by_distance.max(), by_value.max())


def _rho(lam, sigma, n_eig, m):
    d = np.abs(lam - sigma)[_nearest(lam, sigma)]
    return d[n_eig - 1] / d[m] if m < len(lam) else 0.0


def model_near(A, M, X, n_eig, tol, sigma, max_outer):
    """model_eigs of lod_eig_direct_cases.py with the Ritz pairs ordered by |theta - sigma|, ties by ascending theta."""
    import scipy.linalg as sl
    S = A - sigma * M
    theta = res = None
    for outer in range(1, max_outer + 1):
        Z = np.linalg.solve(S, M @ X)
        W, V = A @ Z, M @ Z
        Ga, Gm = Z.T @ W, Z.T @ V
        theta, Q = sl.eigh(0.5 * (Ga + Ga.T), 0.5 * (Gm + Gm.T))
        order = _nearest(theta, sigma)
        theta, Q = theta[order], Q[:, order]
        X = Z @ Q
        AX, MX = W @ Q, V @ Q
        res = np.linalg.norm(AX - MX * theta, axis=0) / (np.abs(theta) * np.linalg.norm(MX, axis=0))
        if (res[:n_eig] <= tol).all():
            break
    return theta, res, outer, X


def _shift_call(c, f, sigma, n_eig, m, X0=None, ld=None, mass=None, **kw):
    """slod_lod_eigs_shift_direct into a NaN-filled block; X0 (numpy [nrow][m]) makes start = 1."""
    ld = m if ld is None else ld
    X = ed._nan(c.nrow, ld)
    if X0 is not None:
        X[:, :m] = ed._dev(X0)
    lam, res, outer = c.g.lod_eigs_shift_direct(f, sigma, c.sym.data_ptr(), (c.mvalues if mass is None else mass).data_ptr(),
                                                c.cols.data_ptr(), n_eig, X.data_ptr(), n_block=m, ld_x=ld,
                                                start=0 if X0 is None else 1, **kw)
    return lam, res, outer, X


def _ldl(c, sigma):
    values, S = lc.shifted_values(c, sigma)
    return c.g.lod_factor_ldl(values.data_ptr(), c.cols.data_ptr())


def _residuals(c, X, theta):
    AX, MX = c.A @ X, c.M @ X
    return np.linalg.norm(AX - MX * theta, axis=0) / (np.abs(theta) * np.linalg.norm(MX, axis=0))


def _residual_floor(c, X, theta, m):
    """The rounding bound of the two evaluations of the normalised residual (test_gpu_lod_eig_direct.py), per column."""
    terms = c.nrow + c.g.lod_row_capacity() * c.s + m + 4
    mag = np.abs(c.A) @ np.abs(X) + (np.abs(c.M) @ np.abs(X)) * np.abs(theta)
    return terms * 2.0 ** -53 * np.linalg.norm(mag, axis=0) / (np.abs(theta) * np.linalg.norm(c.M @ X, axis=0))


# ---- nearest pairs, consistency with the inertia, the outer count

@pytest.mark.parametrize("which", [1, 2])              # shift_at(.., rows / 4), shift_at(.., rows / 2)
@pytest.mark.parametrize("name", PENCILS)
def test_pairs_nearest_an_interior_shift(so, name, which):
    c = lc.ldl_case(so, name)
    label, sigma, below, _ = c.shifts[which]
    n_eig, m = N_EIG, M_BLOCK
    rho = _rho(c.lam, sigma, n_eig, m)
    bound = ed.outer_bound(rho, TOL)
    f = _ldl(c, sigma)
    n_negative = f.inertia().n_negative
    assert n_negative == below
    # from the hashed block: the pairs, their residuals, the inertia
    lam, res, outer, X = _shift_call(c, f, sigma, n_eig, m, max_outer=max(200, 2 * bound))
    hX = X.cpu().numpy()
    err = _nearest_error(lam[:n_eig], c.lam, sigma)
    orth = np.abs(hX.T @ c.M @ hX - np.eye(m)).max()
    ref, floor = _residuals(c, hX, lam), _residual_floor(c, hX, lam, m)
    print("%s %s: sigma %.6e (%d below), rho %.3f: outer %d from the hashed block (bound %d), eigenvalues %s, error %.3e, "
          "|X^T M X - I| %.3e, residuals %s" % (name, label, sigma, below, rho, outer, bound, ["%.8e" % v for v in lam[:n_eig]],
                                                err, orth, ["%.2e" % r for r in res[:n_eig]]))
    assert err <= 1e-8
    assert orth <= 1e-10
    assert (res[:n_eig] <= TOL).all()
    assert (np.diff(np.abs(lam - sigma)) >= 0).all()                 # every column in order of distance
    for j in range(n_eig):
        assert abs(res[j] - ref[j]) <= 1e-6 * ref[j] + floor[j], (j, res[j], ref[j], floor[j])
    converged = res <= TOL
    assert int((lam[converged] < sigma).sum()) <= n_negative
    # the outer count from the caller's block: the model on the CPU first
    X0 = np.random.default_rng(SEED).uniform(-1.0, 1.0, (c.nrow, m))
    model = model_near(c.A, c.M, X0, n_eig, TOL, sigma, bound + 1)[2]
    assert model <= bound, (name, label, model, bound)               # the premise: choose another seed if this fails
    lam1, res1, outer1, X1 = _shift_call(c, f, sigma, n_eig, m, X0=X0, max_outer=bound + 1)
    print("   from default_rng(%d): outer %d, model %d, bound %d" % (SEED, outer1, model, bound))
    assert (res1[:n_eig] <= TOL).all() and _nearest_error(lam1[:n_eig], c.lam, sigma) <= 1e-8
    assert outer1 <= bound
    f.close()


def test_full_spectrum_splits_as_the_inertia_says(so):
    c = lc.ldl_case(so, "dense")
    m = c.nrow
    assert m == 16
    for label, sigma, below, _ in c.shifts:
        f = _ldl(c, sigma)
        n_negative = f.inertia().n_negative
        lam, res, outer, X = _shift_call(c, f, sigma, m, m)
        f.close()
        err = _nearest_error(lam, c.lam, sigma)
        print("dense %s: sigma %.6e, n_negative %d, below sigma among the 16 returned %d, eigenvalue error %.3e, outer %d"
              % (label, sigma, n_negative, int((lam < sigma).sum()), err, outer))
        assert err <= 1e-8 and (res <= TOL).all()
        assert int((lam < sigma).sum()) == n_negative == below


# ---- the start block and repeatability

def test_hashed_start_block_and_repeatability(so):
    import slod_amd
    torch, dev = _torch()
    c = lc.ldl_case(so, "step64")
    label, sigma, below, _ = c.shifts[1]
    f = _ldl(c, sigma)
    m, n_eig = 6, 2
    # with M = 0 the first Ritz step fails (Gm = 0) and d_x holds the block the iteration started from
    zero_mass = torch.zeros_like(c.mvalues)
    X = ed._nan(c.nrow, m + 2)
    with pytest.raises(slod_amd.SlodError) as e:
        c.g.lod_eigs_shift_direct(f, sigma, c.sym.data_ptr(), zero_mass.data_ptr(), c.cols.data_ptr(), n_eig, X.data_ptr(), n_block=m,
                                  ld_x=m + 2, start=0, max_outer=1)
    assert e.value.code == -5 and "slod_lod_eigs_shift_direct" in str(e.value) and "outer iteration 1" in str(e.value)
    assert ed.same_words(X[:, :m].cpu().numpy(), lc.hash_block(c.nrow, m))
    assert bool(torch.isnan(X[:, m:]).all())
    # start = 0 is start = 1 from that block, and a second call gives the same bits
    runs = [_shift_call(c, f, sigma, n_eig, m), _shift_call(c, f, sigma, n_eig, m),
            _shift_call(c, f, sigma, n_eig, m, X0=lc.hash_block(c.nrow, m))]
    f.close()
    l0, r0, o0, x0 = runs[0]
    for l1, r1, o1, x1 in runs[1:]:
        assert ed.same_words(l0, l1) and ed.same_words(r0, r1) and o0 == o1
        assert np.array_equal(_bits(x0), _bits(x1))
    assert (r0[:n_eig] <= TOL).all()


# ---- the definite case: sigma = 0 on either kind of factor

@pytest.mark.parametrize("name", ["step64", "s2"])
def test_shift_zero_agrees_with_the_lowest_pairs(so, name):
    c = lc.ldl_case(so, name)
    n_eig, m = N_EIG, M_BLOCK
    fc = c.g.lod_factor(c.sym.data_ptr(), c.cols.data_ptr())
    fl = c.g.lod_factor_ldl(c.sym.data_ptr(), c.cols.data_ptr())
    low = ed.eigs_direct(c.g, fc, c.sym, c.mvalues, c.cols, c.nrow, n_eig, m)[0]
    for kind, f in (("Cholesky", fc), ("LDL^T", fl)):
        lam, res, outer, X = _shift_call(c, f, 0.0, n_eig, m)
        agree = np.abs(lam[:n_eig] / low[:n_eig] - 1.0).max()
        print("%s sigma = 0 on the %s factor: outer %d, against slod_lod_eigs_direct %.3e" % (name, kind, outer, agree))
        assert agree <= 1e-8 and (res[:n_eig] <= TOL).all()
    fc.close()
    fl.close()


# ---- the ensemble call

@pytest.mark.parametrize("name,K", [("base", 3), ("s2", 3), ("rowmajor", 3), ("base", 65)])
def test_shift_ensemble_members_have_the_words_of_the_single_call(so, name, K):
    import scipy.linalg as sl
    import slod_amd
    torch, dev = _torch()
    c = ed.ensemble_case(so, name)
    g, cols, n_eig, m = c.g, c.cols, 2, 5
    lam0 = sl.eigh(c.A[0], c.M[0], eigvals_only=True)
    sigma = float(0.5 * (lam0[c.nrow // 4 - 1] + lam0[c.nrow // 4]))         # interior for every member; one for all
    A, M = ed.stack(c, c.sym, K, pad=1), ed.stack(c, c.mass, K, pad=2)
    S = ed._nan(c.nval, K)
    g.lod_matrix_combine_ensemble(1.0, A.data_ptr(), -sigma, M.data_ptr(), K, S.data_ptr(), ld_a=K + 1, ld_b=K + 2)
    torch.cuda.synchronize()
    f = g.lod_factor_ldl_ensemble(S.data_ptr(), cols.data_ptr(), K)
    X = ed._nan(c.nrow, K * m + 3)
    lam, res, status, rc = g.lod_eigs_shift_ensemble_direct(f, sigma, A.data_ptr(), M.data_ptr(), cols.data_ptr(), K, n_eig,
                                                            X.data_ptr(), n_block=m, ld_a_m=K + 1, ld_m_m=K + 2, ld_x=K * m + 3,
                                                            max_outer=40)
    assert rc == status.max() and (status >= 1).all()
    assert bool(torch.isnan(X[:, K * m:]).all()) and bool(torch.isfinite(X[:, :K * m]).all())
    xb = _bits(X)
    for k in range(K):
        Ak, Mk, Sk = A[:, k].contiguous(), M[:, k].contiguous(), S[:, k].contiguous()
        fk = g.lod_factor_ldl(Sk.data_ptr(), cols.data_ptr())
        Xk = ed._nan(c.nrow, m)
        l1, r1, o1 = g.lod_eigs_shift_direct(fk, sigma, Ak.data_ptr(), Mk.data_ptr(), cols.data_ptr(), n_eig, Xk.data_ptr(), n_block=m,
                                             max_outer=40)
        fk.close()
        assert status[k] == o1, (name, K, k, status[k], o1)
        assert ed.same_words(lam[k], l1) and ed.same_words(res[k], r1), (name, K, k)
        assert np.array_equal(xb[:, k * m:(k + 1) * m], _bits(Xk)), (name, K, k)
    print("%s K = %d: sigma %.6e, outer per member min %d max %d, n_negative of member 0 %d"
          % (name, K, sigma, status.min(), status.max(), f.inertia(0).n_negative))
    if K == 3:                                                       # a factor of another member count
        with pytest.raises(slod_amd.SlodError) as e:
            g.lod_eigs_shift_ensemble_direct(f, sigma, A.data_ptr(), M.data_ptr(), cols.data_ptr(), 2, n_eig, X.data_ptr(), n_block=m,
                                             ld_a_m=K + 1, ld_m_m=K + 2, ld_x=K * m + 3)
        assert e.value.code == -1 and "slod_lod_eigs_shift_ensemble_direct: factor of another member count" in str(e.value)
    f.close()


# ---- the driver

_driver_pencil = []


def _driver_case(so):
    """The pencil of `main_Diffusion 3 4 1 1` through the Python path, its spectrum and the shift of the rule at rows / 4;
    built once."""
    import scipy.linalg as sl
    if not _driver_pencil:
        cfg = so.make_cfg(nref=3, n_sub=4, oversampling=1, stabilize=1)
        c = _build(so, dict(nref=3, n_sub=4, oversampling=1, spacedim=1),
                   fields=[so.fill_coefficient_rand(1.0, 100.0, 3, so.n_cells_per_side(cfg) * 4, seed=1)])
        c.mvalues, _ = _mass(c)
        c.sym = _symmetrize(c)
        hc = c.cols.cpu().numpy().view(np.uint32)
        c.A = _rows_to_dense(c.g, c.sym.cpu().numpy(), hc, c.s)
        c.M = _rows_to_dense(c.g, c.mvalues.cpu().numpy(), hc, c.s)
        c.perm = lc.factor_order(c)
        c.lam = sl.eigh(c.A, c.M, eigvals_only=True)
        c.sigma, c.below, _ = lc.shift_at(c.lam, c.A, c.M, c.nrow // 4, c.perm)
        _driver_pencil.append(c)
    return _driver_pencil[0]


def _driver(*args):
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "dealii-slod_amd"), "bin/main_Diffusion"])
    r = subprocess.run([BIN, "3", "4", "1", "1", *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return r.stdout


def test_driver_eigs_near_a_shift_matches_python_path(so):
    c = _driver_case(so)
    spectrum, sigma, below = c.lam, c.sigma, c.below
    f = _ldl(c, sigma)
    X = ed._nan(c.nrow, 8)
    lam, res, outer = c.g.lod_eigs_shift_direct(f, sigma, c.sym.data_ptr(), c.mvalues.data_ptr(), c.cols.data_ptr(), 4, X.data_ptr())
    n_negative = f.inertia().n_negative
    f.close()
    out = _driver("--eigs", "4", "--direct", "--shift", repr(sigma), "--ldl")
    pairs = re.findall(r"^eigenvalue (\d+) = (\S+), residual = (\S+)$", out, re.M)
    assert [int(p[0]) for p in pairs] == [1, 2, 3, 4], out
    d_lam, d_res = np.array([float(p[1]) for p in pairs]), np.array([float(p[2]) for p in pairs])
    line = re.findall(r"^factor: n = (\d+), half bandwidth = (\d+), bytes = (\d+), LDL\^T, n_negative = (\d+) \(eigenvalues below "
                      r"sigma\), growth = (\S+)$", out, re.M)
    assert len(line) == 1 and line[0][:2] == ("64", "27"), out
    print("driver: n_negative %s, growth %s, eigenvalues %s; python: n_negative %d, eigenvalues %s"
          % (line[0][3], line[0][4], d_lam, n_negative, lam[:4]))
    assert int(line[0][3]) == n_negative == below
    assert float(line[0][4]) <= lc.GROWTH_CAP
    assert _nearest_error(d_lam, spectrum, sigma) <= 1e-8 and _nearest_error(lam[:4], spectrum, sigma) <= 1e-8
    assert np.abs(np.sort(d_lam) / np.sort(lam[:4]) - 1.0).max() <= 1e-8
    assert (d_res <= TOL).all() and (res[:4] <= TOL).all()


def test_driver_ensemble_eigs_near_a_shift(so):
    """--ensemble 3 --eigs 2 --direct --shift SIGMA --ldl prints per member n_negative, growth and the pairs nearest SIGMA;
    member 0 is the run without --ensemble, to the digits printed; then the mean and standard deviation of n_negative and
    of each eigenvalue over the members."""
    K, N = 3, 2
    sigma = repr(_driver_case(so).sigma)
    out = _driver("--ensemble", str(K), "--eigs", str(N), "--direct", "--shift", sigma, "--ldl")
    lines = re.findall(r"^member (\d+) eigenvalue (\d+) = (\S+), residual = (\S+)$", out, re.M)
    assert [(int(a), int(b)) for a, b, _, _ in lines] == [(k, j) for k in range(K) for j in range(1, N + 1)], out
    assert all(float(r) <= TOL for k, _, _, r in lines if int(k) == 0), out   # sigma is the rule's shift for member 0
    counts = re.findall(r"^member (\d+) factor: n_negative = (\d+), growth = (\S+)$", out, re.M)
    assert [int(k) for k, _, _ in counts] == list(range(K)), out
    below = np.array([int(n) for _, n, _ in counts], dtype=np.float64)
    head = re.findall(r"^factor: n = 64, half bandwidth = 27, bytes = (\d+), LDL\^T, n_negative = (\d+) \(eigenvalues below sigma\), "
                      r"growth = (\S+)$", out, re.M)
    # (the run without --ensemble comes first in the same output: its factor line, then that of the ensemble factor)
    assert len(head) == 2 and all((h[1], h[2]) == (counts[0][1], counts[0][2]) for h in head) and int(head[1][0]) > int(head[0][0]), out
    stat = re.search(r"^n_negative over the ensemble of 3: mean = (\S+), standard deviation = (\S+)$", out, re.M)
    assert stat, out
    assert abs(float(stat.group(1)) - below.mean()) <= 1e-9 and abs(float(stat.group(2)) - below.std(ddof=1)) <= 1e-9
    one = _driver("--eigs", str(N), "--direct", "--shift", sigma, "--ldl")
    pairs = re.findall(r"^eigenvalue (\d+) = (\S+), residual = (\S+)$", one, re.M)
    single = re.search(r"n_negative = (\d+) \(eigenvalues below sigma\), growth = (\S+)$", one, re.M)
    assert len(pairs) == N and single and (single.group(1), single.group(2)) == (counts[0][1], counts[0][2]), one
    for j, lam, res in pairs:
        assert [(l, r) for a, b, l, r in lines if (int(a), int(b)) == (0, int(j))][0] == (lam, res), (j, lam, res)
    stats = re.findall(r"^eigenvalue (\d+) over the ensemble of 3: mean = (\S+), standard deviation = (\S+)$", out, re.M)
    assert [int(t[0]) for t in stats] == [1, 2], out
    for j, mean, std in stats:
        x = np.array([float(l) for a, b, l, r in lines if int(b) == int(j)])
        assert abs(float(mean) / x.mean() - 1.0) <= 1e-6 and abs(float(std) / x.std(ddof=1) - 1.0) <= 1e-5, (j, mean, std)
    print("driver ensemble: n_negative per member %s, growth %s" % (below.tolist(), [g for _, _, g in counts]))
