"""GPU tests of the L2 side of the coarse problem: slod_lod_mass_matrix (M_LOD = C^T M_rho C), slod_lod_apply_multi
(Y = A X), slod_lod_matrix_combine (alpha A + beta B) and slod_lod_theta_steps (theta scheme for M u' + A u = b),
against dense numpy on the same basis, against themselves (bits of a column depend on that column only), and
against the fine FEM heat flow and the fine generalised eigenvalues computed on the CPU.

Tolerances:
  mass entries      1e-12 max|M_ref|   the tolerance test_gpu_lod_system.py uses for A_LOD against Phi Psi^T
  asymmetry         1e-14 max|M|       (the kernel's element form is symmetric bit for bit, so 0 is expected)
  all-ones row sum  1e-14 relative     sums of at most 9 x 36 positive terms, each with a few roundings
  apply             1e-13 max|Y_ref|   rows of at most 49 x 2 products
  stepper           1e-8  max|u_ref|   the tolerance of the existing coarse-solve test, with rel_tol = 1e-13
  eigenvalues       lambda_LOD,k >= lambda_h,k (1 - 1e-8): Courant-Fischer for a subspace, 1e-8 for the symmetrisation
                    of A_LOD (asymmetric to ~1e-9 of its scale, test_lod_system_matches_dense_numpy)
The figures the tests print (mass error and asymmetry, lambda_LOD,1 / lambda_h,1 - 1, the two heat-flow errors) are
recorded in DESIGN section 6, "LOD mass matrix and time stepper".
"""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import make_fields
from lod_cases import (MASS_CONFIGS, _Case, _apply, _bits, _build, _fem_reference, _global_dense, _mass, _mass_fine, _mk,
                       _rows_to_dense, _torch)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dealii-slod_amd", "bin", "main_Diffusion")
UNUSED = 0xffffffff
NAN = float("nan")


def _rho(NE):
    return np.random.default_rng(11).uniform(0.5, 2.0, NE * NE)


@pytest.fixture(scope="module", params=sorted(MASS_CONFIGS))
def mcase(request, so):
    return _build(so, MASS_CONFIGS[request.param])


@pytest.mark.parametrize("density", ["one", "random"])
def test_mass_matrix_matches_dense_numpy(mcase, density):
    """M_LOD against Phi M_h Phi^T with M_h assembled in numpy; the pattern of slod_lod_matrix word for word; exact
    zeros where two patches share only a line of nodes; symmetry; a repeated call gives the same bits."""
    torch, dev = _torch()
    c, g, s = mcase, mcase.g, mcase.s
    rho = None if density == "one" else _rho(g.NE)
    rho_t = None if rho is None else torch.from_numpy(rho).to(dev)
    values, cols = _mass(c, rho_t)
    assert np.array_equal(cols.cpu().numpy().view(np.uint32), c.cols.cpu().numpy().view(np.uint32))
    hv, hc = values.cpu().numpy(), cols.cpu().numpy().view(np.uint32)
    assert np.isfinite(hv).all()
    M = _rows_to_dense(g, hv, hc, s)
    Phi, _ = _global_dense(g, s, c.b.cpu().numpy(), c.q.cpu().numpy(), c.stride)
    Mh = np.kron(_mass_fine(g.NE, rho), np.eye(s))
    Mref = Phi @ Mh @ Phi.T
    scale = np.abs(Mref).max()
    err, asym = np.abs(M - Mref).max(), np.abs(M - M.T).max()
    print("%s rho %s: max |M - Phi M_h Phi^T| = %.3e (max |M| %.3e), asymmetry %.3e" % (c.kw, density, err, scale, asym))
    assert err <= 1e-12 * scale
    assert asym <= 1e-14 * np.abs(M).max()
    # unused slots hold 0; pairs of patches that share only a line of nodes keep their column with the value 0
    cap, n = g.lod_row_capacity(), g.cfg.n_subdivisions
    v4, c2 = hv.reshape(g.num_patches, cap, s, s), hc.reshape(g.num_patches, cap)
    assert (v4[c2 == UNUSED] == 0.0).all()
    info = [g.patch_layout(p) for p in range(g.num_patches)]
    lines = 0
    for p in range(g.num_patches):
        for j in range(cap):
            if c2[p, j] == UNUSED:
                continue
            a, b = info[p], info[int(c2[p, j])]
            w = min(a.x0 + a.mx, b.x0 + b.mx) - max(a.x0, b.x0)
            hgt = min(a.y0 + a.my, b.y0 + b.my) - max(a.y0, b.y0)
            assert w >= 0 and hgt >= 0
            if w == 0 or hgt == 0:
                lines += 1
                assert (v4[p, j] == 0.0).all() and not np.signbit(v4[p, j]).any(), (p, j)
    if n * g.N > (2 * g.cfg.oversampling + 1) * n:       # the domain is wider than one patch: such pairs exist
        assert lines > 0
    again, cols2 = _mass(c, rho_t)
    assert np.array_equal(_bits(again), _bits(values)) and torch.equal(cols2, cols)


@pytest.mark.parametrize("density", ["one", "random"])
def test_mass_matrix_all_ones_counts_elements(so, density):
    """The all-ones slab of the parallel_assembly golden set-up (H = 1/4, n = 2, l = 1, two components): phi = 1 is
    not zero on the rims, so the kernel's value is the element-wise definition restricted to the intersections:
    sum_q M[(p,d),(q,d)] = s sum_{elements e of patch p} rho_e h^2 #(patches that contain e).  This checks the
    intersection arithmetic on its own."""
    torch, dev = _torch()
    cfg, g = _mk(so, nref=2, n_sub=2, oversampling=1, spacedim=2, stabilize=1)
    s, n, NE = 2, 2, g.NE
    c = _Case()
    c.g, c.s, c.ids = g, s, np.arange(g.num_patches, dtype=np.uint32)
    c.stride = g.plan(c.ids).stride
    info = [g.patch_layout(p) for p in range(g.num_patches)]
    hb = np.zeros(g.num_patches * c.stride)
    mult = np.zeros((NE, NE))
    for p, i in enumerate(info):
        hb[p * c.stride:p * c.stride + s * i.n_fine] = 1.0
        mult[i.y0 * n:(i.y0 + i.my) * n, i.x0 * n:(i.x0 + i.mx) * n] += 1.0
    rho = np.ones(NE * NE) if density == "one" else _rho(NE)
    rho_t = None if density == "one" else torch.from_numpy(rho).to(dev)
    values, cols = _mass(c, rho_t, basis=torch.from_numpy(hb).to(dev))
    M = _rows_to_dense(g, values.cpu().numpy(), cols.cpu().numpy().view(np.uint32), s)
    weight = rho.reshape(NE, NE) * mult / (NE * NE)
    for p, i in enumerate(info):
        ref = s * weight[i.y0 * n:(i.y0 + i.my) * n, i.x0 * n:(i.x0 + i.mx) * n].sum()
        for d in range(s):
            got = M[p * s + d, d::s].sum()
            assert abs(got - ref) <= 1e-14 * ref, (p, d, got, ref)


# ---- product and combination

@pytest.fixture(scope="module")
def step_case(so):
    """nref 3, n_sub 2, l = 1, D100: 64 rows (4 groups of 16); stiffness, mass and their symmetrised dense copies."""
    c = _build(so, dict(nref=3, n_sub=2, oversampling=1, spacedim=1))
    c.mvalues, _ = _mass(c)
    hc = c.cols.cpu().numpy().view(np.uint32)
    A = _rows_to_dense(c.g, c.values.cpu().numpy(), hc, 1)
    M = _rows_to_dense(c.g, c.mvalues.cpu().numpy(), hc, 1)
    c.A, c.M = 0.5 * (A + A.T), 0.5 * (M + M.T)
    return c


@pytest.mark.parametrize("which", ["step", "s2"])
def test_apply_matches_dense_and_columns_are_independent(so, step_case, which):
    """Y = A X against the dense product at n_rhs = 1, 3, 65 (65 crosses the 64-column chunk); as 64-bit words a
    column equals the n_rhs = 1 call on it, the call with padded leading dimensions, and its image under a column
    permutation."""
    torch, dev = _torch()
    c = step_case if which == "step" else _build(so, MASS_CONFIGS["s2"])
    A = _rows_to_dense(c.g, c.values.cpu().numpy(), c.cols.cpu().numpy().view(np.uint32), c.s)
    K = 65
    X = torch.from_numpy(np.random.default_rng(3).uniform(-1.0, 1.0, (c.nrow, K))).to(dev)
    Yref = A @ X.cpu().numpy()
    Y65 = _apply(c, c.values, X, K)
    for n in (1, 3, 65):
        Xn = X[:, :n].contiguous()
        Y = _apply(c, c.values, Xn, n)
        err = np.abs(Y.cpu().numpy() - Yref[:, :n]).max()
        print("%s n_rhs %d: max |Y - A X| = %.3e of %.3e" % (which, n, err, np.abs(Yref[:, :n]).max()))
        assert err <= 1e-13 * np.abs(Yref[:, :n]).max()
        assert np.array_equal(_bits(Y), _bits(Y65[:, :n]))
    for k in (0, 2, 63, 64):
        Y1 = _apply(c, c.values, X, 1, first=k)          # column k of the wide array, ld_x = 65, ld_y = 1
        assert np.array_equal(_bits(Y1[:, 0]), _bits(Y65[:, k])), k
    Xw = torch.full((c.nrow, K + 5), NAN, dtype=torch.float64, device=dev)
    Xw[:, :K] = X
    Yw = _apply(c, c.values, Xw, K, ld_y=K + 7)
    assert np.array_equal(_bits(Yw[:, :K]), _bits(Y65)) and bool(torch.isnan(Yw[:, K:]).all())
    perm = torch.from_numpy(np.random.default_rng(5).permutation(K)).to(dev)
    Yp = _apply(c, c.values, X[:, perm].contiguous(), K)
    assert np.array_equal(_bits(Yp), _bits(Y65[:, perm]))


def test_apply_walks_more_groups_than_blocks():
    """32768 rows are 2048 groups of 16 rows, more than the 1024 blocks of a launch: every block walks two groups.
    The product needs no basis, so the matrix is synthetic: 9 random columns per row, the rest unused."""
    import slod_amd
    torch, dev = _torch()
    g = slod_amd.Slod(nref=7, n_sub=1, oversampling=1, spacedim=2)
    NP, cap, s, n = g.num_patches, g.lod_row_capacity(), 2, 3
    rng = np.random.default_rng(17)
    cols = np.full((NP, cap), UNUSED, dtype=np.uint32)
    cols[:, :9] = rng.integers(0, NP, (NP, 9))
    vals = rng.uniform(-1.0, 1.0, (NP, cap, s, s))
    vals[cols == UNUSED] = NAN                         # an unused slot is never multiplied in
    X = rng.uniform(-1.0, 1.0, (NP, s, n))
    Yref = np.einsum("pjde,pjen->pdn", vals[:, :9], X[cols[:, :9].astype(np.int64)])
    vt, ct, xt = torch.from_numpy(vals).to(dev), torch.from_numpy(cols.view(np.int32)).to(dev), torch.from_numpy(X).to(dev)
    Y = torch.zeros_like(xt)
    g.lod_apply(vt.data_ptr(), ct.data_ptr(), xt.data_ptr(), Y.data_ptr(), n_rhs=n)
    torch.cuda.synchronize()
    assert np.abs(Y.cpu().numpy() - Yref).max() <= 1e-13 * np.abs(Yref).max()


def test_combine_matches_numpy_bit_for_bit(step_case):
    """out = (alpha * a) + (beta * b), the form include/slod.h states, is what numpy's alpha * A + beta * B rounds
    to; the output may be either input."""
    torch, dev = _torch()
    c = step_case
    alpha, beta = 0.75, 1.3e-3
    ref = (alpha * c.mvalues.cpu().numpy() + beta * c.values.cpu().numpy()).view(np.uint64)
    out = torch.full_like(c.values, NAN)
    c.g.lod_matrix_combine(alpha, c.mvalues.data_ptr(), beta, c.values.data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out), ref)
    unused = np.repeat(c.cols.cpu().numpy().view(np.uint32) == UNUSED, c.s * c.s)
    assert (out.cpu().numpy()[unused] == 0.0).all()
    for alias in (0, 1):
        a, b = c.mvalues.clone(), c.values.clone()
        c.g.lod_matrix_combine(alpha, a.data_ptr(), beta, b.data_ptr(), (a, b)[alias].data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(_bits((a, b)[alias]), ref), alias
    neg = torch.full_like(c.values, NAN)
    c.g.lod_matrix_combine(-2.0, c.values.data_ptr(), 1.0 / 3.0, c.mvalues.data_ptr(), neg.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(neg.cpu().numpy(), -2.0 * c.values.cpu().numpy() + (1.0 / 3.0) * c.mvalues.cpu().numpy())


# ---- theta stepper

DT, STEPS = 0.01, 3


def _loads(c, n_loads):
    """[n_loads][nrow] coarse loads C^T f_k, f_k = (k + 1) sin((k + 1) pi x) sin(pi y) + 1 at the quadrature points."""
    torch, dev = _torch()
    g = c.g
    g0 = 0.5 * (1.0 - 1.0 / np.sqrt(3.0))
    ey, ex, q = np.meshgrid(np.arange(g.NE), np.arange(g.NE), np.arange(4), indexing="ij")
    x = ((ex + np.where(q & 1, 1.0 - g0, g0)) / g.NE).ravel()
    y = ((ey + np.where(q & 2, 1.0 - g0, g0)) / g.NE).ravel()
    fine = torch.zeros((g.NE + 1) ** 2, dtype=torch.float64, device=dev)
    B = torch.zeros(n_loads, c.nrow, dtype=torch.float64, device=dev)
    for k in range(n_loads):
        fq = torch.from_numpy((k + 1) * np.sin((k + 1) * np.pi * x) * np.sin(np.pi * y) + 1.0).to(dev)
        g.fem_rhs(fq.data_ptr(), fine.data_ptr())
        g.lod_rhs(c.ids, c.b.data_ptr(), c.stride, fine.data_ptr(), B[k].data_ptr())
    torch.cuda.synchronize()
    return B


def _steps(c, theta, n_steps, u, n_rhs=1, load=None, ld_load=None, stride=0, rel_tol=1e-13, dt=DT):
    its, res = c.g.lod_theta_steps(c.values.data_ptr(), c.mvalues.data_ptr(), c.cols.data_ptr(), dt, theta, n_steps,
                                   u.data_ptr(), n_rhs=n_rhs, d_load=None if load is None else load.data_ptr(),
                                   ld_load=ld_load, load_step_stride=stride, rel_tol=rel_tol, max_iterations=5000)
    return its, res


def _reference_steps(c, theta, n_steps, u0, loads, dt=DT):
    """The same recursion with np.linalg.solve on the symmetrised device matrices; loads(k) = b^k."""
    S = c.M + theta * dt * c.A
    u = u0.copy()
    for k in range(n_steps):
        gk = theta * loads(k + 1) + (1.0 - theta) * loads(k) - c.A @ u
        u = u + np.linalg.solve(S, dt * gk)
    return u


@pytest.mark.parametrize("theta", [1.0, 0.5])
@pytest.mark.parametrize("loading", ["constant", "distinct"])
def test_theta_steps_match_dense_recursion(step_case, theta, loading):
    torch, dev = _torch()
    c = step_case
    B = _loads(c, STEPS + 1)
    hB = B.cpu().numpy()
    u0 = np.random.default_rng(23).uniform(-1e-3, 1e-3, c.nrow)
    u = torch.from_numpy(u0).to(dev)
    if loading == "constant":
        its, res = _steps(c, theta, STEPS, u, load=B[1], stride=0)
        uref = _reference_steps(c, theta, STEPS, u0, lambda k: hB[1])
    else:
        its, res = _steps(c, theta, STEPS, u, load=B, stride=c.nrow)
        uref = _reference_steps(c, theta, STEPS, u0, lambda k: hB[k])
    err = np.abs(u.cpu().numpy() - uref).max() / np.abs(uref).max()
    print("theta %.1f, %s load: iterations %s, worst residual %.2e, relative error of u^3 %.3e"
          % (theta, loading, its.tolist(), res.max(), err))
    assert len(its) == STEPS and (its > 0).all() and (its < 5000).all() and (res <= 1e-13).all()
    assert err <= 1e-8


def test_theta_steps_compose_and_columns_are_independent(step_case):
    """One call with n_steps = 2 equals two calls with n_steps = 1; with n_rhs = 3 every column equals its own
    n_rhs = 1 run (different initial states and loads per column, padded leading dimensions); as 64-bit words."""
    torch, dev = _torch()
    c = step_case
    n, theta = 3, 0.5
    B = _loads(c, 3 * n)                                          # 3 time levels x 3 columns
    L = torch.full((3, c.nrow, n + 2), NAN, dtype=torch.float64, device=dev)   # [level][row][column], ld_load = n + 2
    for k in range(3):
        for col in range(n):
            L[k, :, col] = B[k * n + col]
    U0 = torch.full((c.nrow, n + 4), NAN, dtype=torch.float64, device=dev)
    U0[:, :n] = torch.from_numpy(np.random.default_rng(29).uniform(-1e-3, 1e-3, (c.nrow, n))).to(dev)
    U = U0.clone()
    its2, _ = c.g.lod_theta_steps(c.values.data_ptr(), c.mvalues.data_ptr(), c.cols.data_ptr(), DT, theta, 2, U.data_ptr(),
                                  n_rhs=n, ld_u=n + 4, d_load=L.data_ptr(), ld_load=n + 2,
                                  load_step_stride=c.nrow * (n + 2), rel_tol=1e-13, max_iterations=5000)
    assert bool(torch.isnan(U[:, n:]).all()) and bool(torch.isfinite(U[:, :n]).all())
    V = U0.clone()
    its1 = []
    for k in range(2):
        it, _ = c.g.lod_theta_steps(c.values.data_ptr(), c.mvalues.data_ptr(), c.cols.data_ptr(), DT, theta, 1, V.data_ptr(),
                                    n_rhs=n, ld_u=n + 4, d_load=L[k].data_ptr(), ld_load=n + 2,
                                    load_step_stride=c.nrow * (n + 2), rel_tol=1e-13, max_iterations=5000)
        its1.append(int(it[0]))
    assert np.array_equal(_bits(U[:, :n]), _bits(V[:, :n])) and its2.tolist() == its1
    worst = []
    for col in range(n):
        u = U0[:, col].contiguous()
        Lc = L[:, :, col].contiguous()                            # [level][row], ld_load = 1
        it, _ = _steps(c, theta, 2, u, load=Lc, stride=c.nrow)
        assert np.array_equal(_bits(u), _bits(U[:, col])), col
        worst.append(it)
    assert np.array_equal(np.max(np.stack(worst), axis=0), its2)


def test_theta_steps_zero_problem_and_energy_decay(step_case):
    """Zero load and u^0 = 0 give u = 0 and 0 iterations.  With zero load, backward Euler does not increase u^T M u
    from step to step (a property of the scheme for symmetric positive definite M and A): <= up to the rounding
    1e-12 u^T M u."""
    torch, dev = _torch()
    c = step_case
    u = torch.zeros(c.nrow, 2, dtype=torch.float64, device=dev)
    its, res = _steps(c, 1.0, 2, u, n_rhs=2)
    assert its.tolist() == [0, 0] and res.tolist() == [0.0, 0.0]
    assert np.array_equal(_bits(u), np.zeros((c.nrow, 2), np.uint64))
    u = torch.from_numpy(np.random.default_rng(31).uniform(-1.0, 1.0, c.nrow)).to(dev)
    energy = [float(u.cpu().numpy() @ c.M @ u.cpu().numpy())]
    for _ in range(4):
        its, _ = _steps(c, 1.0, 1, u)
        assert its[0] > 0
        energy.append(float(u.cpu().numpy() @ c.M @ u.cpu().numpy()))
    print("u^T M u over 4 backward Euler steps without load:", ["%.6e" % e for e in energy])
    assert energy[0] > 0
    for a, b in zip(energy, energy[1:]):
        assert b <= a + 1e-12 * a


# ---- eigenvalues and the heat flow against the fine space

def test_generalised_eigenvalues_bound_the_fine_ones(so):
    """N = 4, n_sub = 4, l = 2, Poisson with coefficient 1: the LOD space is a subspace of the fine space, so the
    k-th generalised eigenvalue of (A_LOD, M_LOD) is not below the k-th of (A_h, M_h) on the 15^2 interior nodes."""
    import scipy.linalg as sl
    c = _build(so, dict(nref=2, n_sub=4, oversampling=2, spacedim=1), dist="const")
    mvalues, _ = _mass(c)
    hc = c.cols.cpu().numpy().view(np.uint32)
    A = _rows_to_dense(c.g, c.values.cpu().numpy(), hc, 1)
    M = _rows_to_dense(c.g, mvalues.cpu().numpy(), hc, 1)
    A, M = 0.5 * (A + A.T), 0.5 * (M + M.T)
    Linv = np.linalg.inv(np.linalg.cholesky(M))
    lam_lod = np.linalg.eigh(Linv @ A @ Linv.T)[0][:6]
    NE = c.g.NE
    Ah, _, idx = _fem_reference(NE, 1, [np.ones(NE * NE * 4)])
    Mh = _mass_fine(NE)[np.ix_(idx, idx)]
    lam_h = sl.eigh(Ah.toarray(), Mh, eigvals_only=True)[:6]
    print("lambda_LOD", lam_lod, "lambda_h", lam_h, "lambda_LOD,1 / lambda_h,1 - 1 = %.3e" % (lam_lod[0] / lam_h[0] - 1.0))
    assert (lam_h > 0).all()
    assert (lam_lod >= lam_h * (1.0 - 1e-8)).all()


def test_heat_flow_converges_to_fine_heat_flow_with_oversampling(so):
    """N = 8, n_sub = 2, D100, backward Euler, 8 steps, f = 1, u^0 = 0: relative L2 error (slod_compute_error_norms)
    of the reconstructed LOD state at the final time against the fine FEM heat flow run in scipy on the CPU; strictly
    smaller for l = 2 than for l = 1.  The issue leaves dt open: 1e-3, so that at T = 8e-3 the flow has not settled
    on the elliptic solution and the mass matrix still matters.  DESIGN section 6 records both errors."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spl
    torch, dev = _torch()
    dt, steps = 1e-3, 8
    errs = []
    for ell in (1, 2):
        c = _build(so, dict(nref=3, n_sub=2, oversampling=ell, spacedim=1))
        g, NE = c.g, c.g.NE
        cfg = so.make_cfg(nref=3, n_sub=2, oversampling=ell, spacedim=1, stabilize=1)
        Ah, fh, idx = _fem_reference(NE, 1, make_fields(so, cfg, "D100"))
        Mh = sp.csc_matrix(_mass_fine(NE)[np.ix_(idx, idx)])
        solve = spl.factorized((Mh + dt * Ah).tocsc())
        uh = np.zeros(len(idx))
        for _ in range(steps):
            uh = solve(Mh @ uh + dt * fh)
        ref = np.zeros((NE + 1) ** 2)
        ref[idx] = uh
        ref_t = torch.from_numpy(ref).to(dev)
        mvalues, _ = _mass(c)
        f = torch.zeros((NE + 1) ** 2, dtype=torch.float64, device=dev)
        g.fem_rhs(None, f.data_ptr())
        rhs = torch.zeros(c.nrow, dtype=torch.float64, device=dev)
        g.lod_rhs(c.ids, c.b.data_ptr(), c.stride, f.data_ptr(), rhs.data_ptr())
        u = torch.zeros_like(rhs)
        its, res = g.lod_theta_steps(c.values.data_ptr(), mvalues.data_ptr(), c.cols.data_ptr(), dt, 1.0, steps, u.data_ptr(),
                                     d_load=rhs.data_ptr(), rel_tol=1e-13, max_iterations=5000)
        assert (res <= 1e-13).all()
        fine = torch.zeros_like(f)
        g.lod_reconstruct(c.b.data_ptr(), c.stride, u.data_ptr(), fine.data_ptr())
        torch.cuda.synchronize()
        errs.append(g.error_norms(fine.data_ptr(), ref_t.data_ptr())["l2"] / g.error_norms(ref_t.data_ptr())["l2"])
        print("heat flow, l = %d: iterations %s, relative L2 error at T = %g against FEM(h): %.4e"
              % (ell, its.tolist(), dt * steps, errs[-1]))
    assert errs[1] < errs[0], errs


def test_driver_heat_matches_python_path(so):
    """bin/main_Diffusion 3 4 1 1 --heat 4 0.01 (the driver's coefficient Alpha(1, 100, 3), srand(1); f = 1; backward
    Euler from 0) prints the per-step iterations and the error table of the final state against the elliptic SLOD
    solution of the Python path; the error shrinks as STEPS DT grows."""
    torch, dev = _torch()
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "dealii-slod_amd"), "bin/main_Diffusion"])

    def run(steps, dt):
        r = subprocess.run([BIN, "3", "4", "1", "1", "--heat", str(steps), dt], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        its = [int(v) for v in re.findall(r"^heat step \d+: iterations = (\d+)", r.stdout, re.M)]
        resid = [float(v) for v in re.findall(r"^heat step \d+: iterations = \d+, relative residual = (\S+)", r.stdout, re.M)]
        table = r.stdout.split("vs elliptic SLOD solution")[1]
        err = {k: float(v) for k, v in re.findall(r"^  (\S+) +error = (\S+)", table, re.M)}
        rel = {k: float(v) for k, v in re.findall(r"^  (\S+) +error = \S+ +\(relative (\S+)\)", table, re.M)}
        assert len(its) == steps and sorted(err) == sorted(rel) == ["H1", "L2", "Linfty", "energy"], r.stdout
        return its, resid, err, rel

    its, resid, err, rel = run(4, "0.01")
    _, _, longer, _ = run(8, "0.01")
    assert longer["L2"] < err["L2"] and longer["energy"] < err["energy"]
    # the Python path
    cfg = so.make_cfg(nref=3, n_sub=4, oversampling=1, stabilize=1)
    c = _build(so, dict(nref=3, n_sub=4, oversampling=1, spacedim=1),
               fields=[so.fill_coefficient_rand(1.0, 100.0, 3, so.n_cells_per_side(cfg) * 4, seed=1)])
    g = c.g
    mvalues, _ = _mass(c)
    f = torch.zeros((g.NE + 1) ** 2, dtype=torch.float64, device=dev)
    g.fem_rhs(None, f.data_ptr())
    rhs = torch.zeros(c.nrow, dtype=torch.float64, device=dev)
    g.lod_rhs(c.ids, c.b.data_ptr(), c.stride, f.data_ptr(), rhs.data_ptr())
    uH = torch.zeros_like(rhs)
    g.lod_solve(c.values.data_ptr(), c.cols.data_ptr(), rhs.data_ptr(), uH.data_ptr(), 1e-13, 5000)
    u = torch.zeros_like(rhs)
    pits, pres = g.lod_theta_steps(c.values.data_ptr(), mvalues.data_ptr(), c.cols.data_ptr(), 0.01, 1.0, 4, u.data_ptr(),
                                   d_load=rhs.data_ptr(), rel_tol=1e-13, max_iterations=5000)
    fine_e, fine_t = torch.zeros_like(f), torch.zeros_like(f)
    g.lod_reconstruct(c.b.data_ptr(), c.stride, uH.data_ptr(), fine_e.data_ptr())
    g.lod_reconstruct(c.b.data_ptr(), c.stride, u.data_ptr(), fine_t.data_ptr())
    torch.cuda.synchronize()
    e = g.error_norms(fine_e.data_ptr(), fine_t.data_ptr())
    assert its == pits.tolist(), (its, pits)
    assert max(resid) <= 1e-13 and pres.max() <= 1e-13
    # every row of the table, and its relative column (printed with 7 digits) against the norms of the elliptic state
    un = g.error_norms(fine_e.data_ptr())
    for row, key in (("L2", "l2"), ("H1", "h1"), ("Linfty", "linf"), ("energy", "energy")):
        assert err[row] == pytest.approx(e[key], rel=1e-8), row
        assert rel[row] == pytest.approx(e[key] / un[key], rel=2e-6), row
