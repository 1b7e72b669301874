"""GPU tests of slod_lod_matrix_symmetrize and slod_lod_eigs (block inverse iteration with Rayleigh-Ritz on the pencil
(A_LOD, M_LOD)) against dense numpy / scipy on the same block rows.

Tolerances:
  symmetrise         0: the output equals numpy's 0.5 * (A + A.T) as 64-bit words
  eigenvalues        1e-8 relative, the project's tolerance for coarse solves
  X^T M X = I        1e-10
  returned residual  against the one recomputed in numpy from the returned X and theta: 1e-6 relative, or both <= 1e-12
  outer iterations   <= 2 ceil(log tol / log rho) + 5 with rho = lambda_{n_eig} / lambda_{m+1}: the error of block
                     inverse iteration contracts by rho per step, the factor 2 covers the start block and the constant
  invariant subspace ||(I - P_cluster) x_j||_M <= 1e-6.  Clusters are runs of dense eigenvalues whose neighbours are
                     closer than 1e-3 relative: the angle between x_j and the invariant subspace of its cluster is
                     bounded by residual / gap to the rest of the spectrum, 1e-10 / 1e-3 = 1e-7 with the residual
                     normalised as the library does, which leaves a factor 10 for the norm equivalence constants.
The figures the tests print are recorded in DESIGN section 6, "Eigensolver on the LOD space".
"""
import math
import os
import re
import subprocess

import numpy as np
import pytest

from lod_cases import _bits, _build, _fem_reference, _mass, _mass_fine, _pencil, _rows_to_dense, _symmetrize, _torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dealii-slod_amd", "bin", "main_Diffusion")
UNUSED = 0xffffffff
NAN = float("nan")
TOL = 1e-10


def _eigs(c, n_eig, m, start=0, X=None, ld=None, **kw):
    torch, dev = _torch()
    ld = m if ld is None else ld
    if X is None:
        X = torch.full((c.nrow, ld), NAN, dtype=torch.float64, device=dev)
    lam, res, its = c.g.lod_eigs(c.sym.data_ptr(), c.mvalues.data_ptr(), c.cols.data_ptr(), n_eig, X.data_ptr(), n_block=m,
                                 ld_x=ld, start=start, **kw)
    return lam, res, its, X


def _outer_bound(rho, tol=TOL):
    return 5 if rho <= 0.0 else 2 * math.ceil(math.log(tol) / math.log(rho)) + 5


def _block_width(lam, n_eig):
    """The smallest m >= n_eig with rho = lambda_{n_eig} / lambda_{m+1} <= 0.5 (lambda_{rows+1} = infinity), and rho."""
    for m in range(n_eig, len(lam) + 1):
        rho = lam[n_eig - 1] / lam[m] if m < len(lam) else 0.0
        if rho <= 0.5:
            return m, rho
    raise AssertionError("unreachable")


def _residuals(c, X, theta):
    AX, MX = c.A @ X, c.M @ X
    return np.linalg.norm(AX - MX * theta, axis=0) / (np.abs(theta) * np.linalg.norm(MX, axis=0))


def _clusters(lam):
    """Runs of eigenvalues whose neighbours are closer than 1e-3 relative, as a list of index arrays."""
    cuts = np.nonzero(np.diff(lam) > 1e-3 * lam[1:])[0] + 1
    return np.split(np.arange(len(lam)), cuts)


# ---- test 1: symmetrise

@pytest.mark.parametrize("name", ["s1", "s2", "rowmajor"])
def test_symmetrize_equals_numpy_bit_for_bit(so, name):
    import slod_amd
    c = _pencil(so, name)
    g, s, out = c.g, c.s, c.sym
    hc = c.cols.cpu().numpy().view(np.uint32)
    A = _rows_to_dense(g, c.values.cpu().numpy(), hc, s)
    S = _rows_to_dense(g, out.cpu().numpy(), hc, s)
    ref = 0.5 * (A + A.T)
    print("%s: max |out - 0.5 (A + A^T)| = %.3e, skew part of A %.3e of max |A| %.3e"
          % (name, np.abs(S - ref).max(), np.abs(A - A.T).max(), np.abs(A).max()))
    assert np.array_equal(S.view(np.uint64), ref.view(np.uint64))
    assert np.array_equal(S.view(np.uint64), np.ascontiguousarray(S.T).view(np.uint64))
    unused = np.repeat(hc == UNUSED, s * s)
    assert unused.any() and (_bits(out)[unused] == 0).all()            # +0, not -0 and not the NaN fill
    with pytest.raises(slod_amd.SlodError) as e:
        g.lod_matrix_symmetrize(c.values.data_ptr(), c.cols.data_ptr(), c.values.data_ptr())
    assert e.value.code == -1


# ---- test 2: full spectrum, m = rows: the Gram, Ritz and rotate kernels on their own

@pytest.mark.parametrize("name", ["s1", "rowmajor", "step64", "s2"])
def test_full_spectrum_matches_dense(so, name):
    c = _pencil(so, name)
    m = c.nrow
    assert m == {"s1": 16, "rowmajor": 25, "step64": 64, "s2": 32}[name]
    lam, res, its, X = _eigs(c, m, m)
    hX = X.cpu().numpy()
    err = np.abs(lam / c.lam - 1.0).max()
    orth = np.abs(hX.T @ c.M @ hX - np.eye(m)).max()
    ref = _residuals(c, hX, lam)
    print("%s m = rows = %d: outer %d, inner %s, max eigenvalue error %.3e, max |X^T M X - I| %.3e, residuals max %.3e "
          "(recomputed %.3e), lambda_max / lambda_1 = %.3e" % (name, m, len(its), its.tolist(), err, orth, res.max(), ref.max(),
                                                             c.lam[-1] / c.lam[0]))
    assert (np.diff(lam) >= 0).all()
    assert err <= 1e-8
    assert orth <= 1e-10
    for j in range(m):
        assert abs(res[j] - ref[j]) <= 1e-6 * ref[j] or (res[j] <= 1e-12 and ref[j] <= 1e-12), (j, res[j], ref[j])


# ---- test 3: the lowest pairs with guard columns

@pytest.mark.parametrize("n_eig", [1, 2, 6])
@pytest.mark.parametrize("name", ["step64", "const"])
def test_lowest_pairs_with_guards(so, name, n_eig):
    c = _pencil(so, name)
    m, rho = _block_width(c.lam, n_eig)
    assert m <= 64
    lam, res, its, X = _eigs(c, n_eig, m)
    hX = X.cpu().numpy()
    err = np.abs(lam[:n_eig] / c.lam[:n_eig] - 1.0).max()
    bound = _outer_bound(rho)
    # distance of x_j from the invariant subspace of the cluster of lambda_j, in the M-norm
    dist = []
    for j in range(n_eig):
        idx = next(k for k in _clusters(c.lam) if j in k)
        Vc = c.vec[:, idx]
        r = hX[:, j] - Vc @ (Vc.T @ (c.M @ hX[:, j]))
        dist.append(math.sqrt(max(r @ c.M @ r, 0.0)))
    print("%s n_eig %d, m %d, rho %.3f: outer %d (bound %d), inner %s, eigenvalue error %.3e, residuals %s, "
          "subspace distance %.3e" % (name, n_eig, m, rho, len(its), bound, its.tolist(), err,
                                      ["%.2e" % r for r in res[:n_eig]], max(dist)))
    assert err <= 1e-8
    assert (res[:n_eig] <= TOL).all()
    assert len(its) <= bound
    assert max(dist) <= 1e-6


def test_single_vector_inverse_iteration(so):
    """n_eig = 1, m = 1 on the 16-row case: plain inverse iteration, rho = lambda_1 / lambda_2."""
    c = _pencil(so, "s1")
    rho = c.lam[0] / c.lam[1]
    lam, res, its, X = _eigs(c, 1, 1)
    x = X.cpu().numpy()[:, 0]
    print("m = 1: rho %.3f, outer %d (bound %d), eigenvalue error %.3e, residual %.2e"
          % (rho, len(its), _outer_bound(rho), abs(lam[0] / c.lam[0] - 1.0), res[0]))
    assert abs(lam[0] / c.lam[0] - 1.0) <= 1e-8 and res[0] <= TOL
    assert len(its) <= _outer_bound(rho)
    assert abs(x @ c.M @ x - 1.0) <= 1e-10


def test_eigenvalues_bound_the_fine_ones(so):
    """Coefficient 1, N = 4, n_sub = 4, l = 2: theta_k >= lambda_h,k (1 - 1e-8), k <= 6, as the dense path of
    test_generalised_eigenvalues_bound_the_fine_ones asserts."""
    import scipy.linalg as sl
    c = _pencil(so, "const")
    m, _ = _block_width(c.lam, 6)
    lam, res, its, _ = _eigs(c, 6, m)
    NE = c.g.NE
    Ah, _, idx = _fem_reference(NE, 1, [np.ones(NE * NE * 4)])
    Mh = _mass_fine(NE)[np.ix_(idx, idx)]
    lam_h = sl.eigh(Ah.toarray(), Mh, eigvals_only=True)[:6]
    print("lambda_LOD", lam[:6], "lambda_h", lam_h, "lambda_LOD,1 / lambda_h,1 - 1 = %.3e" % (lam[0] / lam_h[0] - 1.0))
    assert (res[:6] <= TOL).all()
    assert (lam[:6] >= lam_h * (1.0 - 1e-8)).all()


# ---- test 4: the caller's start block, leading dimension, repeatability, a rank-deficient block

def test_callers_start_block_ld_and_repeatability(so):
    import slod_amd
    torch, dev = _torch()
    c = _pencil(so, "step64")
    n_eig = 2
    m, rho = _block_width(c.lam, n_eig)
    X0 = torch.full((c.nrow, m + 3), NAN, dtype=torch.float64, device=dev)
    X0[:, :m] = torch.from_numpy(np.random.default_rng(41).uniform(-1.0, 1.0, (c.nrow, m))).to(dev)
    lam, res, its, X = _eigs(c, n_eig, m, start=1, X=X0.clone(), ld=m + 3)
    assert bool(torch.isnan(X[:, m:]).all()) and bool(torch.isfinite(X[:, :m]).all())
    assert np.abs(lam[:n_eig] / c.lam[:n_eig] - 1.0).max() <= 1e-8 and (res[:n_eig] <= TOL).all()
    # the same call twice, and the library's start block twice
    for start in (1, 0):
        runs = [_eigs(c, n_eig, m, start=start, X=X0.clone(), ld=m + 3) for _ in range(2)]
        (l0, r0, i0, x0), (l1, r1, i1, x1) = runs
        assert np.array_equal(l0.view(np.uint64), l1.view(np.uint64)) and np.array_equal(r0.view(np.uint64), r1.view(np.uint64))
        assert i0.tolist() == i1.tolist()
        assert np.array_equal(_bits(x0[:, :m]), _bits(x1[:, :m]))
    # two equal columns: Gm = Z^T M Z is singular
    Xd = X0.clone()
    Xd[:, m - 1] = Xd[:, 0]                                        # inside the block for every m >= 2 (index m is padding)
    with pytest.raises(slod_amd.SlodError) as e:
        _eigs(c, n_eig, m, start=1, X=Xd, ld=m + 3)
    assert e.value.code == -5 and "pivot" in str(e.value) and "slod_lod_eigs" in str(e.value)


# ---- test 5: more slabs than blocks

def test_gram_and_rotate_walk_more_slabs_than_blocks():
    """32768 rows are 1024 slabs of the Gram kernel (512 blocks) and 2048 of the rotate kernel (1024 blocks).  A
    diagonal pencil needs no basis: A = M lambda with lambda = 1, 2, 3, 4 at four rows (first slab, last slab, two
    interior ones that a block reaches on its second pass) and lambda in [100, 200] elsewhere."""
    import slod_amd
    torch, dev = _torch()
    g = slod_amd.Slod(nref=7, n_sub=1, oversampling=1, spacedim=2)
    NP, cap, s = g.num_patches, g.lod_row_capacity(), 2
    nrow = NP * s
    assert nrow == 32768
    rng = np.random.default_rng(43)
    mass = rng.uniform(0.5, 2.0, nrow)
    lam = rng.uniform(100.0, 200.0, nrow)
    special = [5, 513 * 32 + 7, 700 * 32 + 2, nrow - 4]               # two rows of each component
    lam[special] = [1.0, 2.0, 3.0, 4.0]
    cols = np.full((NP, cap), UNUSED, dtype=np.uint32)
    cols[:, 0] = np.arange(NP)
    mv = np.zeros((NP, cap, s, s))
    av = np.zeros((NP, cap, s, s))
    for d in range(s):
        mv[:, 0, d, d] = mass[d::s]
        av[:, 0, d, d] = (mass * lam)[d::s]
    ct = torch.from_numpy(cols.view(np.int32)).to(dev)
    mt, at = torch.from_numpy(mv).to(dev), torch.from_numpy(av).to(dev)
    m, n_eig = 8, 4
    X = torch.full((nrow, m), NAN, dtype=torch.float64, device=dev)
    th, res, its = g.lod_eigs(at.data_ptr(), mt.data_ptr(), ct.data_ptr(), n_eig, X.data_ptr(), n_block=m)
    hX = X.cpu().numpy()
    bound = _outer_bound(4.0 / 100.0)
    worst = 0.0
    for j, r in enumerate(special):
        e = np.zeros(nrow)
        e[r] = 1.0 / math.sqrt(mass[r])
        worst = max(worst, min(np.abs(hX[:, j] - e).max(), np.abs(hX[:, j] + e).max()))
    print("diagonal pencil: theta %s, residuals %s, outer %d (bound %d), inner %s, max |x_j -+ e_r / sqrt(M_rr)| = %.3e"
          % (th[:n_eig], res[:n_eig], len(its), bound, its.tolist(), worst))
    assert np.abs(th[:n_eig] - np.array([1.0, 2.0, 3.0, 4.0])).max() <= 1e-10
    assert (res[:n_eig] <= TOL).all()
    assert worst <= 1e-8
    assert len(its) <= bound


# ---- test 6: one outer iteration is a result, not an error

def test_max_outer_one(so):
    c = _pencil(so, "step64")
    lam, res, its, X = _eigs(c, 2, 8, max_outer=1)
    assert len(its) == 1 and its[0] > 0
    assert np.isfinite(res).all() and np.isfinite(lam).all() and np.isfinite(X.cpu().numpy()).all()


# ---- test 7: the driver

def test_driver_eigs_matches_python_path(so):
    """bin/main_Diffusion 3 4 1 1 --eigs 4 (the driver's coefficient Alpha(1, 100, 3), srand(1)) against the Python
    path on the same coefficient with the same defaults."""
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "dealii-slod_amd"), "bin/main_Diffusion"])
    r = subprocess.run([BIN, "3", "4", "1", "1", "--eigs", "4"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    pairs = re.findall(r"^eigenvalue (\d+) = (\S+), residual = (\S+)$", r.stdout, re.M)
    assert [int(p[0]) for p in pairs] == [1, 2, 3, 4], r.stdout
    d_lam, d_res = np.array([float(p[1]) for p in pairs]), np.array([float(p[2]) for p in pairs])
    counts = re.search(r"^eigensolver: outer iterations = (\d+), inner iterations =((?: \d+)+)$", r.stdout, re.M)
    assert counts, r.stdout
    d_outer, d_inner = int(counts.group(1)), [int(v) for v in counts.group(2).split()]
    norms = [float(v) for v in re.findall(r"^eigenfunction \d+: L2 norm = (\S+)$", r.stdout, re.M)]
    assert len(norms) == 4 and all(v > 0.0 for v in norms), r.stdout
    # the Python path
    torch, dev = _torch()
    cfg = so.make_cfg(nref=3, n_sub=4, oversampling=1, stabilize=1)
    c = _build(so, dict(nref=3, n_sub=4, oversampling=1, spacedim=1),
               fields=[so.fill_coefficient_rand(1.0, 100.0, 3, so.n_cells_per_side(cfg) * 4, seed=1)])
    c.mvalues, _ = _mass(c)
    c.sym = _symmetrize(c)
    X = torch.full((c.nrow, 8), NAN, dtype=torch.float64, device=dev)
    lam, res, its = c.g.lod_eigs(c.sym.data_ptr(), c.mvalues.data_ptr(), c.cols.data_ptr(), 4, X.data_ptr())
    assert len(lam) == 8                                               # the default block: n_eig + max(4, n_eig // 2)
    print("driver eigenvalues", d_lam, "python", lam[:4], "outer", d_outer, "inner", d_inner)
    assert np.abs(d_lam / lam[:4] - 1.0).max() <= 1e-8
    assert d_outer == len(its) and d_inner == its.tolist()
    assert (d_res <= TOL).all() and (res[:4] <= TOL).all()
    # the eigenfunctions are M-orthonormal, and x^T M_LOD x is the squared L2 norm of C x
    assert np.abs(np.array(norms) - 1.0).max() <= 1e-6
